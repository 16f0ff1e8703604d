"""GPU: the VAE decoder from a host with no Python and no torch in the process -- examples/vae_host.cpp is built with hipcc (only
for hipMalloc / hipMemcpy) and run against the in-tree libnesr_hip.so: nesr_vae_create with the `two_levels` configuration, the
weights from a flat file, nesr_vae_decode_latents_u8 on one set of latents.  The frame it writes is the Python result, bit for bit."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import vae_cases as C
from tests.test_gpu_vae_cases import DEV, model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_host_decodes_latents(tmp_path, cuda_device):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available on this box")
    exe = str(tmp_path / "vae_host")
    subprocess.run([hipcc, "-O2", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "vae_host.cpp"), "-o", exe, "-ldl"], check=True, timeout=300)
    lib = os.path.join(ROOT, "neural_enhanced_super_resolution_amd", "libnesr_hip.so")
    case = C.by_name("two_levels")
    np.concatenate([v.numpy().reshape(-1) for v in case.sd.values()]).astype(np.float32).tofile(tmp_path / "weights.f32")
    case.latents.numpy().astype(np.float32).tofile(tmp_path / "latents.f32")
    out = subprocess.run(["timeout", "-k", "10", "60", exe, lib, str(tmp_path / "weights.f32"), str(tmp_path / "latents.f32"), "5", "7",
                          str(tmp_path / "out.ppm"), "16,32", "4", "1"], capture_output=True, text=True, timeout=90)
    assert out.returncode == 0, out.stdout + out.stderr
    print(out.stdout)
    assert f"{len(case.sd)} tensors" in out.stdout and "latents 5 x 7 -> 10 x 14 in 49 launches" in out.stdout
    data = (tmp_path / "out.ppm").read_bytes()
    head = b"P6\n14 10\n255\n"
    assert data.startswith(head) and len(data) == len(head) + 10 * 14 * 3
    got = torch.from_numpy(np.frombuffer(data[len(head):], np.uint8).reshape(10, 14, 3).copy())
    want = model("two_levels").decode_latents_u8(case.latents.to(DEV)).cpu()
    assert torch.equal(got, want)

"""GPU: the UNet's fp16 compute form from a host with no Python and no torch in the process -- examples/unet_host.cpp with
``--dtype fp16`` (nesr_unet_set_dtype between create and finalize) on the `batch_two` configuration.  The result it writes is the
Python result of ``UNet2DCondition(compute_dtype="fp16")``, bit for bit; without the option its output is the f32 form's."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from neural_enhanced_super_resolution_amd import UNet2DCondition
from neural_enhanced_super_resolution_amd.unet import launches_per_forward
from tests import unet_cases as C
from tests.test_gpu_unet_cases import DEV

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_host_runs_an_fp16_forward(tmp_path, cuda_device):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available on this box")
    exe = str(tmp_path / "unet_host")
    subprocess.run([hipcc, "-O2", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "unet_host.cpp"), "-o", exe, "-ldl"], check=True, timeout=300)
    lib = os.path.join(ROOT, "neural_enhanced_super_resolution_amd", "libnesr_hip.so")
    case = C.by_name("batch_two")
    np.concatenate([v.numpy().reshape(-1) for v in case.sd.values()]).astype(np.float32).tofile(tmp_path / "weights.f32")
    case.sample.numpy().astype(np.float32).tofile(tmp_path / "sample.f32")
    case.text.numpy().astype(np.float32).tofile(tmp_path / "text.f32")
    line = [exe, lib, str(tmp_path / "weights.f32"), str(tmp_path / "sample.f32"), str(tmp_path / "text.f32"), "2", "6", "10", "7", str(case.timestep),
            str(case.label), str(tmp_path / "out.f32"), "16,32", "1,1", "1,0", "4", "2", "1", "40", "10"]
    results = {}
    for dtype, extra in (("fp16", ["--dtype", "fp16"]), ("f32", [])):
        out = subprocess.run(["timeout", "-k", "10", "60"] + line[:1] + extra + line[1:], capture_output=True, text=True, timeout=90)
        assert out.returncode == 0, out.stdout + out.stderr
        print(out.stdout)
        assert f"-> [4, 6, 10] in {launches_per_forward(**case.cfg)} launches" in out.stdout and ("compute form: fp16" in out.stdout) == (dtype == "fp16")
        got = torch.from_numpy(np.fromfile(tmp_path / "out.f32", np.float32).reshape(2, 4, 6, 10).copy())
        m = UNet2DCondition(compute_dtype=dtype, **case.cfg).to(DEV)
        m.load_state_dict(case.sd)
        assert torch.equal(got, m(case.sample.to(DEV), case.timestep, case.text.to(DEV), case.label).cpu()), dtype
        results[dtype] = got
    assert not torch.equal(results["fp16"], results["f32"])
    bad = subprocess.run([exe, "--dtype", "bf16"] + line[1:], capture_output=True, text=True, timeout=30)
    assert bad.returncode == 1 and "--dtype takes f32 or fp16" in bad.stderr

"""GPU: one iteration of the pipeline from a host with no Python and no torch in the process -- examples/pipeline_host.cpp is built
with hipcc (only for hipMalloc / hipMemcpy) and run against the in-tree libnesr_hip.so: nesr_preprocess_u8, nesr_stage_route,
nesr_apply_esrgan_u8 (the tiler with its Lanczos paste), nesr_postprocess_u8, nesr_check_range.  Its output file is
nesr_adapter.enhance_iterations(filters=True, one iteration) on the same seeded frame and weights, bit for bit."""
import math
import os
import shutil
import subprocess
from collections import OrderedDict

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mix(seed, i):
    """examples/pipeline_host.cpp's mix(): lowbias32 of the counter."""
    h = (i.astype(np.uint64) + np.uint64((seed * 0x9E3779B9) & 0xFFFFFFFF)) & np.uint64(0xFFFFFFFF)
    for shift, mul in ((16, 0x7feb352d), (15, 0x846ca68b)):
        h ^= h >> np.uint64(shift)
        h = (h * np.uint64(mul)) & np.uint64(0xFFFFFFFF)
    return (h ^ (h >> np.uint64(16))).astype(np.uint32)


def _uniform(seed, start, n):
    h = _mix(seed, np.arange(start, start + n, dtype=np.uint64))
    return (h >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0) * np.float32(2.0) - np.float32(1.0)


def host_state_dict(seed):
    """The weights examples/pipeline_host.cpp draws, in its order (state_dict order, a layer's weight before its bias)."""
    from neural_enhanced_super_resolution_amd.rrdbnet import rrdbnet_state_dict_spec
    sd, counter = OrderedDict(), 0
    for key, shape in rrdbnet_state_dict_spec(12, 3, 4, 64, 1, 32).items():
        n = int(np.prod(shape))
        u = _uniform(seed, counter, n)
        counter += n
        if key.endswith(".weight"):
            gain = 0.7 if key.startswith("body.") else 1.0
            v = u * np.float32(gain / math.sqrt(shape[1] * 9))
        else:
            v = u * np.float32(0.02) + np.float32(0.5 if key == "conv_last.bias" else 0.0)
        sd[key] = torch.from_numpy(v.astype(np.float32).reshape(shape))
    return sd


def host_frame(seed, h, w):
    i = np.arange(h * w * 3, dtype=np.uint64).reshape(h, w, 3)
    y, x, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing="ij")
    noise = (_mix(seed + 1, i) >> np.uint32(29)).astype(np.int64) * 4
    return ((x * 5 + y * 3 + c * 61 + noise) & 255).astype(np.uint8)


def test_cpp_host_equals_enhance_iterations(tmp_path, cuda_device):
    from neural_enhanced_super_resolution_amd import RRDBNet
    from neural_enhanced_super_resolution_amd import nesr_adapter as A
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available on this box")
    exe = str(tmp_path / "pipeline_host")
    subprocess.run([hipcc, "-O2", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "pipeline_host.cpp"), "-o", exe, "-ldl"], check=True, timeout=300)
    lib = os.path.join(ROOT, "neural_enhanced_super_resolution_amd", "libnesr_hip.so")
    seed, h, w, tile, thr = 5, 40, 56, 24, 0.001                     # 2 x 3 tiles, canvas 80 x 112: every tile through the Lanczos paste
    out = subprocess.run(["timeout", "-k", "10", "120", exe, lib, str(h), str(w), str(tile), str(thr), str(seed), str(tmp_path / "out.rgb")],
                         capture_output=True, text=True, timeout=150)
    assert out.returncode == 0, out.stdout + out.stderr
    print(out.stdout)
    assert "tiled, 6 tiles, 12-channel" in out.stdout

    class Up:
        model = RRDBNet(12, 3, num_block=1)
        device = torch.device(cuda_device)

    Up.model.load_state_dict(host_state_dict(seed))
    Up.model.to(cuda_device)
    trace = []
    want = A.enhance_iterations(Up, host_frame(seed, h, w), {"iterations": 1, "max_tile_size": tile, "cuda_megapixel_threshold": thr}, filters=True, trace=trace)
    assert trace[0]["tiled"] and not trace[0]["three_channel"] and trace[0]["model_calls"] == 6
    got = np.fromfile(tmp_path / "out.rgb", np.uint8).reshape(2 * h, 2 * w, 3)
    assert want.shape == got.shape and np.array_equal(got, want)

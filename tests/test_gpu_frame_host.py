"""GPU: nesr_enhance_frame from a host with no Python and no torch in the process -- examples/frame_host.cpp is built with hipcc (only
for hipMalloc / hipMemcpy) and run against the in-tree libnesr_hip.so on a 16-bit gray frame and an 8-bit BGRA frame; its outputs
are RealESRGANer.enhance's on the same frames, bit for bit.  And the refusals of nesr_enhance_frame that read a context, which
tests/test_frame_io_host.py cannot make without a device."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_host_equals_enhance(tmp_path, cuda_device):
    from neural_enhanced_super_resolution_amd import RealESRGANer, RRDBNet
    from neural_enhanced_super_resolution_amd.synth import synthetic_frame, synthetic_state_dict
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available on this box")
    exe = str(tmp_path / "frame_host")
    subprocess.run([hipcc, "-O2", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "frame_host.cpp"), "-o", exe, "-ldl"], check=True, timeout=300)
    sd = synthetic_state_dict(seed=3, num_in_ch=3, scale=2, num_block=2)
    np.concatenate([v.numpy().reshape(-1) for v in sd.values()]).astype(np.float32).tofile(tmp_path / "weights.f32")
    gray = synthetic_frame(48, 64, seed=2, channels=0).astype(np.uint16) * 251
    bgra = np.concatenate([synthetic_frame(36, 44, seed=3), synthetic_frame(36, 44, seed=4, channels=0)[:, :, None]], 2)
    gray.tofile(tmp_path / "gray16.raw")
    bgra.tofile(tmp_path / "bgra8.raw")
    lib = os.path.join(ROOT, "neural_enhanced_super_resolution_amd", "libnesr_hip.so")
    out = subprocess.run([exe, lib, str(tmp_path / "weights.f32"), str(tmp_path / "gray16.raw"), "48", "64", str(tmp_path / "gray16_out.raw"),
                          str(tmp_path / "bgra8.raw"), "36", "44", str(tmp_path / "bgra8_out.raw")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    print(out.stdout)
    up = RealESRGANer(scale=2, model_path={"params_ema": sd}, model=RRDBNet(3, 3, scale=2, num_block=2), tile=0, pre_pad=0, half=False, device=cuda_device)
    want_gray, mode = up.enhance(gray)
    assert mode == "L" and want_gray.dtype == np.uint16
    got_gray = np.fromfile(tmp_path / "gray16_out.raw", np.uint16).reshape(96, 128)
    assert np.array_equal(got_gray, want_gray)
    want_bgra, mode = up.enhance(bgra)
    assert mode == "RGBA" and want_bgra.dtype == np.uint8
    got_bgra = np.fromfile(tmp_path / "bgra8_out.raw", np.uint8).reshape(72, 88, 4)
    assert np.array_equal(got_bgra, want_bgra)


def test_entry_equals_enhance_for_compact_plain_alpha_and_dark_frames(cuda_device):
    """The entry through ctypes on the contexts of live models: SRVGGNetCompact, the linear alpha, through_fp16, the dark uint16 frame."""
    import torch
    from neural_enhanced_super_resolution_amd import RealESRGANer, _lib, frame_io
    from tests.test_gpu_frame_io import _frame, _wrapper
    lib = _lib.load()
    for net, kind, hw in (("compact", "bgra16", (20, 28)), ("x2", "bgra8_plain", (24, 28)), ("x2", "dark16", (24, 28)), ("x2_half", "gray8", (24, 28)),
                          ("x4", "bgr16", (17, 23))):
        up = _wrapper(net, cuda_device, tile=0, tile_pad=10, pre_pad=0)
        img, alpha = _frame(kind, hw[0], hw[1], seed=9)
        want, _ = up.enhance(img, alpha_upsampler=alpha)
        ctx = up.model._context(torch.device(cuda_device), 0)
        channels = 1 if img.ndim == 2 else img.shape[2]
        max_range, _ = RealESRGANer._frame_kind(img)
        mode = _lib.ALPHA_LINEAR if alpha != "realesrgan" else _lib.ALPHA_NETWORK
        src = frame_io.frame_to_tensor(img, cuda_device)
        need = lib.nesr_frame_scratch_bytes(ctx, hw[0], hw[1], channels, mode)
        assert need > 0
        scratch = torch.empty(need, dtype=torch.uint8, device=cuda_device)
        dst = torch.empty(want.shape, dtype=torch.uint8 if want.dtype == np.uint8 else torch.int16, device=cuda_device)
        stream = ctypes.c_void_p(torch.cuda.current_stream(cuda_device).cuda_stream)
        _lib.check(lib.nesr_enhance_frame(ctx, ctypes.c_void_p(src.data_ptr()), hw[0], hw[1], channels, img.dtype.itemsize * 8, max_range, mode,
                                          1 if up.half else 0, ctypes.c_void_p(scratch.data_ptr()), need, ctypes.c_void_p(dst.data_ptr()), stream),
                   "nesr_enhance_frame")
        got = frame_io.frame_to_numpy(dst.cpu())
        up.model.check_range()
        assert got.dtype == want.dtype and np.array_equal(got, want), (net, kind)


def test_refusals_that_read_the_context(cuda_device):
    import torch
    from neural_enhanced_super_resolution_amd import RRDBNet, _lib
    from neural_enhanced_super_resolution_amd.synth import synthetic_state_dict
    lib = _lib.load()
    fake = [ctypes.c_void_p(0x1000 * i) for i in (1, 2, 3)]         # never dereferenced: every call fails its argument check first

    def refused(rc, text):
        assert rc == -1 and text in lib.nesr_last_error().decode(), lib.nesr_last_error().decode()

    def ctx_of(num_in_ch, scale):
        m = RRDBNet(num_in_ch, 3, scale=scale, num_block=1)
        m.load_state_dict(synthetic_state_dict(seed=1, num_in_ch=num_in_ch, scale=scale, num_block=1))
        m.to(cuda_device)
        return m, m._context(torch.device(cuda_device), 0)

    m2, x2 = ctx_of(3, 2)
    refused(lib.nesr_enhance_frame(x2, fake[0], 9, 12, 1, 8, 255, 0, 0, fake[1], 1 << 30, fake[2], None), "unshuffle factor 2")
    refused(lib.nesr_enhance_frame(x2, fake[0], 8, 13, 4, 16, 65535, 1, 0, fake[1], 1 << 30, fake[2], None), "unshuffle factor 2")
    assert lib.nesr_frame_scratch_bytes(x2, 9, 12, 1, 0) == 0
    need = lib.nesr_frame_scratch_bytes(x2, 8, 12, 4, 0)
    assert need >= (3 * 8 * 12 + 3 * 16 * 24) * 4 * 2 and need > lib.nesr_frame_scratch_bytes(x2, 8, 12, 4, 1) > lib.nesr_frame_scratch_bytes(x2, 8, 12, 3, 0)
    refused(lib.nesr_enhance_frame(x2, fake[0], 8, 12, 4, 8, 255, 0, 0, fake[1], need - 1, fake[2], None), "scratch")
    refused(lib.nesr_enhance_frame(x2, fake[0], 8, 12, 4, 8, 255, 0, 0, ctypes.c_void_p(0x1010), need, fake[2], None), "256-byte aligned")
    m12, x12 = ctx_of(12, 4)                                          # the 12-channel network of nesr/nesr.py: not an image-to-image one
    refused(lib.nesr_enhance_frame(x12, fake[0], 8, 12, 3, 8, 255, 0, 0, fake[1], 1 << 30, fake[2], None), "3-channel-in")
    assert lib.nesr_frame_scratch_bytes(x12, 8, 12, 3, 0) == 0

"""GPU: the pipeline's Lab conversions, Gaussian blur, adaptive unsharp mask and the whole pre-filter as HIP kernels
(csrc/filters.hip, csrc/filters_api.cpp) -- each bit for bit the torch chain of imgproc.py it replaces (use_hip=False), which
tests/test_imgproc.py and tests/test_gpu_filters.py pin against oracle/cv2_ref.py.  PARITY UNPINNED against OpenCV (absent)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _all_triples(dev):
    """4096 x 4096 x 3 uint8 holding every (c0, c1, c2) once."""
    i = torch.arange(1 << 24, device=dev, dtype=torch.int32)
    return torch.stack([i >> 16, (i >> 8) & 255, i & 255], -1).to(torch.uint8).reshape(4096, 4096, 3)


def _textured(h, w, seed, dev):
    """Smooth colour ramps plus noise: flat and detailed regions both occur."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randint(0, 256, (1, 3, h // 16 + 2, w // 16 + 2), generator=g).float()
    img = torch.nn.functional.interpolate(base, size=(h, w), mode="bilinear", align_corners=False)[0].permute(1, 2, 0)
    img = img + torch.randint(-20, 21, img.shape, generator=g) * (torch.rand(h, w, 1, generator=g) > 0.5)
    return img.clamp(0, 255).to(torch.uint8).contiguous().to(dev)


def _differences(got, want, what):
    bad = (got != want).any(-1) if got.dim() == 3 else (got != want)
    n = int(bad.sum())
    if n:
        idx = bad.nonzero()[:5].tolist()
        return f"{what}: {n} pixels differ, first at {idx}"
    return None


@pytest.mark.parametrize("linear,blue", [(False, False), (True, True), (True, False), (False, True)])
def test_lab_every_input_both_directions(cuda_device, linear, blue):
    from neural_enhanced_super_resolution_amd import imgproc as P
    x = _all_triples(cuda_device)
    for fn in (P.rgb2lab_u8, P.lab2rgb_u8):
        got = fn(x, linear, blue)
        want = fn(x, linear, blue, use_hip=False)
        msg = _differences(got, want, f"{fn.__name__}(linear={linear}, first_is_blue={blue})")
        assert msg is None, msg
    planes = P.rgb2lab_u8(x, linear, blue, planar=True)
    assert planes.shape == (3, 4096, 4096)
    assert torch.equal(planes, P.rgb2lab_u8(x, linear, blue).permute(2, 0, 1))
    assert torch.equal(P.lab2rgb_u8(planes, linear, blue, planar=True), P.lab2rgb_u8(planes.permute(1, 2, 0), linear, blue))
    assert torch.equal(P.lab2rgb_u8(planes, linear, blue, planar=True), P.lab2rgb_u8(planes, linear, blue, use_hip=False, planar=True))


@pytest.mark.parametrize("hw", [(1, 1), (1, 37), (37, 1), (2, 2), (7, 5), (1000, 1777)])
@pytest.mark.parametrize("C", [1, 3])
def test_gaussian_is_the_torch_chain(cuda_device, hw, C):
    from neural_enhanced_super_resolution_amd import imgproc as P
    from oracle import cv2_ref as O
    img = _textured(hw[0], hw[1], seed=hw[0] * 7 + hw[1] + C, dev=cuda_device)
    x = img[..., 1].contiguous() if C == 1 else img
    for sigma, ksize in ((2.0, 0), (3.0, 0), (0.0, 1), (0.0, 3), (0.0, 5), (0.0, 7), (1.2, 31)):
        got = P.gaussian_blur_u8(x, sigma, ksize)
        want = P.gaussian_blur_u8(x, sigma, ksize, use_hip=False)
        assert torch.equal(got, want), (sigma, ksize, _differences(got, want, "gaussian"))
        if hw[0] * hw[1] <= 64:
            assert np.array_equal(got.cpu().numpy(), O.gaussian_blur_u8(x.cpu().numpy(), sigma, ksize))


@pytest.mark.parametrize("hw", [(1, 1), (3, 4), (9, 9), (1000, 1777), (4096, 4096)])
def test_postprocess_is_the_torch_chain(cuda_device, hw):
    from neural_enhanced_super_resolution_amd import imgproc as P
    img = _textured(hw[0], hw[1], seed=3, dev=cuda_device)
    got = P.postprocess_image(img)
    want = P.postprocess_image(img, use_hip=False)
    msg = _differences(got, want, "postprocess")
    assert msg is None, msg
    if hw[0] * hw[1] >= 81:
        assert not torch.equal(got, img)              # some pixels are sharpened
    assert P.postprocess_image(img, adaptive_sharpening=False) is img


def _frames(dev, golden_dir):
    from neural_enhanced_super_resolution_amd.synth import synthetic_frame
    crop = np.load(os.path.join(golden_dir, "test_jpeg_crop_64x96_bgr.npy"))
    return [torch.from_numpy(np.ascontiguousarray(synthetic_frame(18, 22, seed=5)[:, :, ::-1])).to(dev),
            torch.from_numpy(np.ascontiguousarray(crop)).to(dev),
            _textured(1000, 1777, seed=8, dev=dev)]


@pytest.mark.parametrize("level", [0.0, 0.5, 1.0])
def test_preprocess_is_the_all_torch_chain(cuda_device, golden_dir, level):
    from neural_enhanced_super_resolution_amd import imgproc as P
    for img in _frames(cuda_device, golden_dir):
        got = P.preprocess_image(img, level)
        want = P.preprocess_image(img, level, use_hip=False)
        msg = _differences(got, want, f"preprocess {tuple(img.shape)} level {level}")
        assert msg is None, msg
        assert not torch.equal(got, img)


def test_default_route_is_hip(cuda_device, monkeypatch):
    """With the torch helpers of every chain made to raise, the default calls on a device tensor still work: they never
    reach torch.  (use_hip=False does reach them.)"""
    from neural_enhanced_super_resolution_amd import imgproc as P

    def boom(*a, **k):
        raise AssertionError("torch chain used")
    img = _textured(40, 52, seed=1, dev=cuda_device)
    for name in ("_srgb_to_linear", "_linear_to_srgb", "_lab_f", "rgb2gray_u8", "_reflect101_index", "nl_means_weights", "gaussian_kernel_u8"):
        monkeypatch.setattr(P, name, boom)
    P.rgb2lab_u8(img)
    P.lab2rgb_u8(img, True, True)
    P.gaussian_blur_u8(img, 3.0)
    P.gaussian_blur_u8(img[..., 0].contiguous(), 2.0)
    P.preprocess_image(img, 0.5)
    P.postprocess_image(img)
    with pytest.raises(AssertionError, match="torch chain"):
        P.postprocess_image(img, use_hip=False)
    with pytest.raises(AssertionError, match="torch chain"):
        P.rgb2lab_u8(img, use_hip=False)


def test_iteration_with_filters_equals_the_torch_chains(cuda_device, monkeypatch):
    """One enhance_iterations(filters=True) iteration (nesr/nesr.py:516-633): the HIP filters by default, bit for bit the same
    run with every filter forced onto its torch chain."""
    from neural_enhanced_super_resolution_amd import RealESRGANer, RRDBNet, imgproc as P, nesr_adapter as A
    from neural_enhanced_super_resolution_amd.synth import synthetic_frame, synthetic_state_dict
    sd = synthetic_state_dict(seed=6, num_in_ch=12, scale=4, num_block=1)
    up = RealESRGANer(scale=2, model_path={"params_ema": sd}, model=RRDBNet(12, 3, num_block=1), tile=0, tile_pad=0, pre_pad=0,
                      half=False, device=cuda_device)
    img = synthetic_frame(18, 22, seed=5)[:, :, ::-1].copy()
    cfg = {"iterations": 1, "upscale_factor": 2.0}
    got = A.enhance_iterations(up, img, cfg, "cuda", filters=True)
    pre, post = P.preprocess_image, P.postprocess_image
    monkeypatch.setattr(P, "preprocess_image", lambda im, level: pre(im, level, use_hip=False))
    monkeypatch.setattr(P, "postprocess_image", lambda im, on: post(im, on, use_hip=False))
    want = A.enhance_iterations(up, img, cfg, "cuda", filters=True)
    assert got.shape == want.shape == (72, 88, 3)
    assert np.array_equal(got, want)


def _side_stream_calls(img):
    from neural_enhanced_super_resolution_amd import imgproc as P
    return [P.preprocess_image(img, 0.5), P.postprocess_image(img), P.gaussian_blur_u8(img, 3.0), P.rgb2lab_u8(img),
            P.lab2rgb_u8(img)]


def test_calls_on_a_side_stream(cuda_device):
    """The entries enqueue on the caller's current stream: their input is produced on a side stream behind a long spin
    kernel and read with no synchronisation in between; an entry that launched on another stream would read it early."""
    img = _textured(300, 411, seed=4, dev=cuda_device)
    ref = _side_stream_calls(img)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=cuda_device)
    with torch.cuda.stream(side):
        x = torch.zeros_like(img)
        torch.cuda._sleep(200_000_000)                   # ~0.1 s of spinning on the side stream
        x.copy_(img)                                    # the input exists only after the spin
        got = _side_stream_calls(x)
        default_idle = torch.cuda.default_stream(cuda_device).query()
    side.synchronize()
    assert default_idle                                 # nothing of it was enqueued on the default stream
    for a, b in zip(got, ref):
        assert torch.equal(a, b)


def test_forced_route_refuses_wrong_layouts_on_the_device(cuda_device):
    from neural_enhanced_super_resolution_amd import imgproc as P
    img = _textured(2, 9, seed=6, dev=cuda_device)
    for call in (lambda: P.postprocess_image(img[..., 0].contiguous(), use_hip=True),
                 lambda: P.postprocess_image(img[..., :1].contiguous(), use_hip=True),
                 lambda: P.lab2rgb_u8(img, planar=True, use_hip=True),               # [2, 9, 3] is no [3, H, W]
                 lambda: P.rgb2lab_u8(img.float(), use_hip=True),
                 lambda: P.gaussian_blur_u8(img[None], 2.0, use_hip=True)):
        with pytest.raises(ValueError, match="HIP kernel takes"):
            call()
    # a sigma with no kernel keeps the torch chain's behaviour on the default route
    with pytest.raises(Exception) as torch_err:
        P.gaussian_blur_u8(img, -1.0, use_hip=False)
    with pytest.raises(type(torch_err.value)):
        P.gaussian_blur_u8(img, -1.0)


def test_preprocess_refuses_small_scratch(cuda_device):
    from neural_enhanced_super_resolution_amd import _lib
    lib = _lib.load()
    img = _textured(20, 30, seed=2, dev=cuda_device)
    need = lib.nesr_preprocess_scratch_bytes(20, 30)
    scratch = torch.empty((need,), dtype=torch.uint8, device=cuda_device)
    out = torch.empty_like(img)
    p = lambda t: ctypes.c_void_p(t.data_ptr())                                         # noqa: E731
    assert lib.nesr_preprocess_u8(0, p(img), 20, 30, 0.5, p(scratch), need - 1, p(out), None) == -1
    assert b"scratch" in lib.nesr_last_error()
    assert lib.nesr_preprocess_u8(0, p(img), 20, 30, 0.5, p(scratch), need, p(out), None) == 0
    torch.cuda.synchronize()
    from neural_enhanced_super_resolution_amd import imgproc as P
    assert torch.equal(out, P.preprocess_image(img, 0.5, use_hip=False))


def test_host_without_torch_runs_the_filters(tmp_path, cuda_device):
    """examples/filters_host.cpp (no Python, no torch in its process) against the torch chains."""
    from neural_enhanced_super_resolution_amd import imgproc as P
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "filters_host")
    subprocess.run([hipcc, "-O2", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "filters_host.cpp"), "-o", exe, "-ldl"], check=True, timeout=300)
    lib = os.path.join(ROOT, "neural_enhanced_super_resolution_amd", "libnesr_hip.so")
    img = _textured(61, 83, seed=12, dev="cpu")
    src = tmp_path / "in.rgb"
    src.write_bytes(img.numpy().tobytes())
    pre, post = tmp_path / "pre.rgb", tmp_path / "post.rgb"
    out = subprocess.run([exe, lib, str(src), "61", "83", "0.5", str(pre), str(post)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    want_pre = P.preprocess_image(img.to(cuda_device), 0.5, use_hip=False)
    want_post = P.postprocess_image(want_pre, use_hip=False)
    got_pre = np.frombuffer(pre.read_bytes(), np.uint8).reshape(61, 83, 3)
    got_post = np.frombuffer(post.read_bytes(), np.uint8).reshape(61, 83, 3)
    assert np.array_equal(got_pre, want_pre.cpu().numpy())
    assert np.array_equal(got_post, want_post.cpu().numpy())

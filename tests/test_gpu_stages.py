"""GPU: the rest of enhance_image's loop as HIP kernels (csrc/resize.hip: nesr_resize_cv_u8; csrc/filters.hip:
nesr_segment_enhance_u8, nesr_ensemble_u8) -- each bit for bit the torch chain of imgproc.py it replaces (use_hip=False), which
tests/test_stages_host.py pins against tests/cv2_stages_ref.py on the CPU.  Every comparison is an equality.  PARITY UNPINNED against
OpenCV (absent)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEAREST, LINEAR, CUBIC, LANCZOS4 = 0, 1, 2, 4
INTERPS = (NEAREST, LINEAR, CUBIC, LANCZOS4)
# where the kernels can go wrong, not where the workload is: one pixel, fewer samples than taps, a single column, the tile edges in
# both axes, a shrink, cv2's area switch, many tiles
SIZES = [((1, 1), (1, 1)), ((1, 1), (9, 5)), ((3, 2), (7, 5)), ((37, 1), (5, 1)), ((66, 130), (131, 259)), ((131, 259), (33, 65)),
         ((128, 192), (64, 96)), ((1000, 1777), (555, 999))]


def _img(h, w, c, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (h, w, c), dtype=torch.uint8, generator=g).to(dev)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize("src,dst", SIZES)
@pytest.mark.parametrize("C", [1, 3, 4])
def test_resize_kernel_is_the_torch_chain(cuda_device, src, dst, C):
    from neural_enhanced_super_resolution_amd import imgproc as P
    img = _img(src[0], src[1], C, seed=src[0] + 7 * dst[1] + C, dev=cuda_device)
    for interp in INTERPS:
        got = P.resize_u8(img, dst[0], dst[1], interp)
        want = P.resize_u8(img, dst[0], dst[1], interp, use_hip=False)
        assert got.shape == want.shape == (dst[0], dst[1], C)
        bad = (got != want).any(-1)
        assert not bad.any(), f"interp {interp}: {int(bad.sum())} pixels differ, first at {bad.nonzero()[:5].tolist()}"


def test_default_route_is_the_kernel(cuda_device, monkeypatch):
    """With the chain's table builder made to raise, the default calls on a device tensor still work; use_hip=False reaches it."""
    from neural_enhanced_super_resolution_amd import imgproc as P
    img = _img(20, 30, 3, seed=1, dev=cuda_device)

    def boom(*a, **k):
        raise AssertionError("torch chain used")
    monkeypatch.setattr(P, "resize_u8_tables", boom)
    monkeypatch.setattr(P, "dilate3x3_u8", boom)
    for interp in (NEAREST, LINEAR, CUBIC):
        P.resize_u8(img, 41, 17, interp)
    P.segment_enhance(img, torch.ones((3, 4), dtype=torch.int64))
    P.ensemble_results([img, img.clone()])
    with pytest.raises(AssertionError, match="torch chain"):
        P.resize_u8(img, 41, 17, CUBIC, use_hip=False)
    with pytest.raises(AssertionError, match="torch chain"):
        P.segment_enhance(img, torch.ones((3, 4), dtype=torch.int64), use_hip=False)


@pytest.mark.parametrize("interp", INTERPS)
def test_rectangle_of_a_canvas_through_row_strides(cuda_device, interp):
    """A 40 x 50 rectangle of a 64 x 80 canvas filled with 0xA5, from a rectangle of a larger source: no byte outside it changes."""
    from neural_enhanced_super_resolution_amd import imgproc as P
    for C in (1, 3, 4):
        frame = _img(50, 61, C, seed=3 + C, dev=cuda_device)
        canvas = torch.full((64, 80, C), 0xA5, dtype=torch.uint8, device=cuda_device)
        region = frame[5:38, 7:52]
        r = P.resize_u8(region, 40, 50, interp, out=canvas[11:51, 13:63])
        assert r.data_ptr() == canvas[11:51, 13:63].data_ptr()
        want = torch.full((64, 80, C), 0xA5, dtype=torch.uint8, device=cuda_device)
        want[11:51, 13:63] = P.resize_u8(region.contiguous(), 40, 50, interp, use_hip=False)
        assert torch.equal(canvas, want)


def test_interp_4_is_nesr_resize_u8(cuda_device):
    from neural_enhanced_super_resolution_amd import _lib
    lib = _lib.load()
    img = _img(66, 130, 3, seed=9, dev=cuda_device)
    a = torch.empty((131, 259, 3), dtype=torch.uint8, device=cuda_device)
    b = torch.empty_like(a)
    torch.cuda.synchronize()
    assert lib.nesr_resize_cv_u8(0, _p(img), 66, 130, 3, 390, _p(a), 131, 259, 777, LANCZOS4, None) == 0
    assert lib.nesr_resize_u8(0, _p(img), 66, 130, 3, 390, _p(b), 131, 259, 777, LANCZOS4, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(a, b)


def _mask(shape, density, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) < density).to(torch.int64).to(dev)


SEG_CASES = [((1, 1), (1, 1), 1.0), ((5, 7), (2, 2), 0.5), ((70, 130), (18, 33), 0.3), ((257, 129), (257, 129), 0.05),
             ((70, 130), (18, 33), 0.5), ((70, 130), (18, 33), 0.0), ((70, 130), (18, 33), 1.0), ((64, 96), (128, 192), 0.5)]


@pytest.mark.parametrize("frame,mask,density", SEG_CASES)
def test_segment_enhance_is_the_torch_chain(cuda_device, frame, mask, density):
    """Frame and mask sizes: one pixel; a mask smaller than the dilate; several tiles; a mask of the frame's size (no resize); random,
    all-0 and all-1 masks; a mask twice the frame (the area switch inside the stage)."""
    from neural_enhanced_super_resolution_amd import imgproc as P
    img = _img(frame[0], frame[1], 3, seed=frame[0] + mask[1], dev=cuda_device)
    seg = _mask(mask, density, seed=mask[0] + int(density * 10), dev=cuda_device) * 5
    got = P.segment_enhance(img, seg)
    want = P.segment_enhance(img, seg, use_hip=False)
    bad = (got != want).any(-1)
    assert not bad.any(), f"{int(bad.sum())} pixels differ, first at {bad.nonzero()[:5].tolist()}"
    if density == 0.0:
        assert torch.equal(got, img)
    if density == 1.0:
        assert torch.equal(got, torch.round(img.float() * 1.5 - P.gaussian_blur_u8(img, 3.0).float() * 0.5).clamp_(0, 255).to(torch.uint8))
    assert torch.equal(P.segment_enhance(img, seg.cpu().numpy().astype(np.int16)), got)          # a host map of another dtype


def test_stages_on_a_side_stream(cuda_device):
    """The entries enqueue on the caller's current stream: their inputs are produced on a side stream behind a long spin and read
    with no synchronisation in between."""
    from neural_enhanced_super_resolution_amd import imgproc as P
    img = _img(70, 130, 3, seed=4, dev=cuda_device)
    other = _img(70, 130, 3, seed=5, dev=cuda_device)
    seg = _mask((18, 33), 0.4, seed=6, dev=cuda_device)

    def calls(x):
        return [P.segment_enhance(x, seg), P.ensemble_results([x, other]), P.resize_u8(x, 33, 200, CUBIC), P.resize_u8(x, 35, 65, LINEAR),
                P.resize_u8(x, 140, 260, NEAREST)]
    ref = calls(img)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=cuda_device)
    with torch.cuda.stream(side):
        x = torch.zeros_like(img)
        torch.cuda._sleep(200_000_000)
        x.copy_(img)
        got = calls(x)
        default_idle = torch.cuda.default_stream(cuda_device).query()
    side.synchronize()
    assert default_idle
    for a, b in zip(got, ref):
        assert torch.equal(a, b)


@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_ensemble_is_the_torch_chain(cuda_device, n):
    """67 x 131 x 3 = 26331 bytes: the 16-byte path has a tail of 11; and the same images at a pointer one byte off (the byte path)."""
    from neural_enhanced_super_resolution_amd import _lib, imgproc as P
    imgs = [_img(67, 131, 3, seed=30 + k, dev=cuda_device) for k in range(n)]
    got = P.ensemble_results(imgs)
    want = P.ensemble_results(imgs, use_hip=False)
    if n == 1:
        assert got is imgs[0]
    assert torch.equal(got, want)
    total = 67 * 131 * 3
    holder = [torch.empty((total + 16,), dtype=torch.uint8, device=cuda_device) for _ in range(n + 1)]
    for h, im in zip(holder, imgs):
        h[1:1 + total] = im.reshape(-1)
    holder[n].fill_(0xA5)
    assert all(h.data_ptr() % 16 == 0 for h in holder)
    ptrs = (ctypes.c_void_p * n)(*[h.data_ptr() + 1 for h in holder[:n]])
    torch.cuda.synchronize()
    assert _lib.load().nesr_ensemble_u8(0, ptrs, n, 67, 131, 3, ctypes.c_void_p(holder[n].data_ptr() + 1), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(holder[n][1:1 + total], want.reshape(-1))
    assert int(holder[n][0]) == 0xA5 and (holder[n][1 + total:] == 0xA5).all()                 # nothing outside the image


_LOOP = {}


def _loop_parts(dev):
    from neural_enhanced_super_resolution_amd import RealESRGANer, RRDBNet, SRVGGNetCompact, nesr_adapter as A
    from neural_enhanced_super_resolution_amd.synth import synthetic_compact_state_dict, synthetic_frame, synthetic_state_dict
    if not _LOOP:
        sd = synthetic_state_dict(seed=6, num_in_ch=12, scale=4, num_block=2)
        _LOOP["up"] = RealESRGANer(scale=2, model_path={"params_ema": sd}, model=RRDBNet(12, 3, num_block=2), tile=0, tile_pad=0, pre_pad=0,
                                   half=False, device=dev)
        cfg = dict(num_in_ch=3, num_out_ch=3, num_feat=64, num_conv=2, upscale=2, act_type="prelu")
        compact = RealESRGANer(scale=2, model_path={"params": synthetic_compact_state_dict(seed=5, **cfg)}, model=SRVGGNetCompact(**cfg),
                               tile=0, pre_pad=0, half=False, device=dev)
        _LOOP["compact"] = compact
        _LOOP["extra"] = A.realesrganer_stage(compact)
        _LOOP["img"] = synthetic_frame(24, 32, seed=5)[:, :, ::-1].copy()
    return _LOOP


def _segmenter(frame):
    return (frame[:, :, 1] > 120).to(torch.int32)


def test_loop_default_route_equals_the_chains(cuda_device):
    """enhance_iterations, two iterations, with a thresholding segmenter and a RealESRGANer around a 2-conv x2 SRVGGNetCompact beside
    the 2-block RRDBNet: the default route (every stage a HIP kernel) against use_hip=False (every stage its torch chain)."""
    from neural_enhanced_super_resolution_amd import nesr_adapter as A
    p = _loop_parts(cuda_device)
    cfg = {"iterations": 2, "upscale_factor": 2.0}
    rr0, cc0 = p["up"].model.calls, p["compact"].model.calls
    t_hip, t_chain = [], []
    got = A.enhance_iterations(p["up"], p["img"], cfg, "cuda", trace=t_hip, filters=True, segmenter=_segmenter, extra_upscalers=[p["extra"]])
    want = A.enhance_iterations(p["up"], p["img"], cfg, "cuda", trace=t_chain, filters=True, segmenter=_segmenter, extra_upscalers=[p["extra"]],
                                use_hip=False)
    assert got.shape == want.shape == (384, 512, 3)
    assert np.array_equal(got, want)
    assert t_hip == t_chain
    assert [(t["iteration"], t["segmented"], t["ensemble_n"], t["model_calls"], t["out_shape"]) for t in t_hip] == \
        [(0, True, 2, 1, (96, 128)), (1, True, 2, 1, (384, 512))]
    assert p["up"].model.calls - rr0 == 4 and p["compact"].model.calls - cc0 == 4              # both networks ran, in both runs


def test_extra_stage_is_enhance_without_the_trip_home(cuda_device):
    """realesrganer_stage(up)(rgb) = up.enhance(bgr)[0] flipped back."""
    p = _loop_parts(cuda_device)
    rgb = torch.from_numpy(p["img"]).to(cuda_device)
    got = p["extra"](rgb).cpu().numpy()
    want = p["compact"].enhance(np.ascontiguousarray(p["img"][:, :, ::-1]))[0][:, :, ::-1]
    assert got.shape == (48, 64, 3) and np.array_equal(got, want)


def test_loop_defaults_are_untouched(cuda_device):
    """With the new arguments left out: the bytes and the trace of the stage's own route (tests/test_gpu_nesr_stage.py), iteration by
    iteration, and no new trace key."""
    from neural_enhanced_super_resolution_amd import nesr_adapter as A
    p = _loop_parts(cuda_device)
    cfg = {"iterations": 2, "upscale_factor": 2.0}
    trace = []
    got = A.enhance_iterations(p["up"], p["img"], cfg, "cuda", trace=trace)
    stage_trace = []
    cur = p["img"]
    for it in range(2):
        cur = A.apply_esrgan(p["up"], cur, dict(cfg, iterations=2), "cuda", as_numpy=False, trace=stage_trace)
        stage_trace[-1]["iteration"] = it
    assert np.array_equal(got, cur.cpu().numpy())
    assert trace == stage_trace and all("segmented" not in t and "ensemble_n" not in t for t in trace)
    assert [t["model_calls"] for t in trace] == [1, 1]
    none = A.enhance_iterations(None, p["img"], {"iterations": 1, "upscale_factor": 2.0}, device=cuda_device)
    from neural_enhanced_super_resolution_amd import imgproc as P
    assert np.array_equal(none, P.resize_u8(torch.from_numpy(p["img"]), 48, 64, CUBIC).numpy())    # the kernel = the CPU chain


def _fnv1a(buf):
    h = 14695981039346656037
    for b in bytes(buf):
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def _seeded(n, seed, mask):
    out = np.empty(n, np.uint8)
    s = seed
    for i in range(n):
        s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
        out[i] = (s >> 24) & mask
    return out


def test_host_without_torch_runs_the_stages(tmp_path, cuda_device):
    """examples/stages_host.cpp in a fresh child process (no Python, no torch in it): its checksums are those of the Python results."""
    from neural_enhanced_super_resolution_amd import imgproc as P
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "stages_host")
    subprocess.run([hipcc, "-O2", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "stages_host.cpp"), "-o", exe, "-ldl"], check=True, timeout=300)
    lib = os.path.join(ROOT, "neural_enhanced_super_resolution_amd", "libnesr_hip.so")
    H, W, MH, MW = 37, 53, 9, 14
    out = subprocess.run([exe, lib, str(H), str(W), str(MH), str(MW)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    sums = dict(line.split() for line in out.stdout.splitlines()[1:])
    frame = torch.from_numpy(_seeded(H * W * 3, 1, 255).reshape(H, W, 3)).to(cuda_device)
    second = torch.from_numpy(_seeded(H * W * 3, 3, 255).reshape(H, W, 3)).to(cuda_device)
    mask = torch.from_numpy(_seeded(MH * MW, 2, 1).reshape(MH, MW).astype(np.int64))
    want = {}
    for name, interp in (("nearest", NEAREST), ("linear", LINEAR), ("cubic", CUBIC), ("lanczos4", LANCZOS4)):
        want[name + "_up"] = P.resize_u8(frame, 2 * H + 1, 2 * W - 1, interp, use_hip=False)
        want[name + "_down"] = P.resize_u8(frame, H // 2 + 1, W // 2 + 2, interp, use_hip=False)
    want["segment"] = P.segment_enhance(frame, mask, use_hip=False)
    want["ensemble"] = P.ensemble_results([frame, second], use_hip=False)
    assert sorted(sums) == sorted(want)
    for name, t in want.items():
        assert int(sums[name], 16) == _fnv1a(t.cpu().numpy().tobytes()), name

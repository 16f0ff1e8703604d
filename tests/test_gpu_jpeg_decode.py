"""GPU: the JPEG decoder's kernels (csrc/jpeg_decode.hip through imgproc.decode_jpeg_u8 and nesr_jpeg_decode_u8) against the
specification (tests/jpeg_decode_ref.py, pinned to libjpeg-turbo in tests/test_jpeg_decode_spec.py).  Every pixel criterion is
equality.  The grid is tests/jpeg_decode_cases.py's, boundary files included; tests/test_jpeg_decode_spec.py proves from the
specification's counters which paths it takes."""
import ctypes
import io
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import jpeg_cases, jpeg_decode_cases as dc, jpeg_decode_ref as ref

pytestmark = pytest.mark.gpu
CASES = dc.cases()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _where(got, want):
    if got.shape != want.shape:
        return f"shape {got.shape} against {want.shape}"
    bad = np.argwhere(got != want)
    return f"{len(bad)} samples differ, the first at {tuple(bad[0]) if len(bad) else None}"


# ------------------------------------------------------------------------------------------------ 7: the grid
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_kernel_pixels_equal_the_specification(cuda_device, case):
    from neural_enhanced_super_resolution_amd import imgproc
    data = dc.file_bytes(*case[1:])
    h, w, c = case[2:5]
    for order in ("rgb", "bgr"):
        want = dc.spec_pixels(data, order)
        got = imgproc.decode_jpeg_u8(data, order=order, device=cuda_device)
        assert got.dtype == torch.uint8 and got.device.type == "cuda" and tuple(got.shape) == want.shape
        assert np.array_equal(got.cpu().numpy(), want), (order, _where(got.cpu().numpy(), want))
        assert torch.equal(imgproc.decode_jpeg_u8(data, order=order, device=cuda_device), got), "the same call twice"
        # into rows 3 .. 3 + h, columns 5 .. 5 + w of a larger tensor filled with another value
        big = torch.full((h + 7, w + 11) + ((3,) if c == 3 else ()), 201, dtype=torch.uint8, device=cuda_device)
        window = big[3:3 + h, 5:5 + w]
        out = imgproc.decode_jpeg_u8(data, order=order, out=window)
        assert out.data_ptr() == window.data_ptr()
        host = big.cpu().numpy()
        assert np.array_equal(host[3:3 + h, 5:5 + w], want), (order, "window")
        host[3:3 + h, 5:5 + w] = 201
        assert (host == 201).all(), "bytes outside the window were written"


LONG = [dc.long_scan, dc.many_mcus]


@pytest.mark.parametrize("build", LONG, ids=[b.__name__ for b in LONG])
def test_long_files_take_a_second_step_of_the_scans(cuda_device, build):
    """A scan of more than 1024 unstuff chunks (jd_scan_chunks carries) and a frame of more than 1024 DC groups (jd_dc_scan carries),
    against Pillow's pixels (tests/test_jpeg_decode_spec.py pins the specification to them); the path is asserted from the host parser
    so that a changed constant cannot leave it untested"""
    from neural_enhanced_super_resolution_amd import _lib, imgproc
    cid, data, want = build()
    info = _lib.jpeg_parse(data)
    nchunks = -(-info.scan_bytes // dc.kernel_constant("jpeg_decode_kernels.h", "UNSTUFF_CHUNK"))
    dc_groups = -(-(info.mcus_x * info.mcus_y) // dc.kernel_constant("jpeg_decode_kernels.h", "DC_GROUP"))
    assert info.restart_interval == 0 and (nchunks if build is dc.long_scan else dc_groups) > dc.SCAN_LANES
    got = imgproc.decode_jpeg_u8(data, device=cuda_device, use_hip=True).cpu().numpy()
    assert np.array_equal(got, want), _where(got, want)


# ------------------------------------------------------------------------------------------------ 8: the reference's asset
def test_reference_asset(cuda_device):
    """512 x 512, 4:2:0, DRI = 32, tables from the file: the pixels the reference's own read recorded."""
    from neural_enhanced_super_resolution_amd import imgproc
    with open(dc.REFERENCE_ASSET, "rb") as f:
        data = f.read()
    want = np.load(os.path.join(jpeg_cases.GOLDEN, "test_jpeg_full.npz"))["input_bgr"]
    got = imgproc.decode_jpeg_u8(data, order="bgr", device=cuda_device, use_hip=True)
    assert np.array_equal(got.cpu().numpy(), want), _where(got.cpu().numpy(), want)


def test_committed_files(cuda_device):
    from neural_enhanced_super_resolution_amd import imgproc
    for entry in dc.GOLDEN_FILES:
        name = dc.golden_name(*entry)
        with open(name + ".jpg", "rb") as f:
            data = f.read()
        assert np.array_equal(imgproc.decode_jpeg_u8(data, device=cuda_device, use_hip=True).cpu().numpy(), np.load(name + ".npy")), name


# ------------------------------------------------------------------------------------------------ 9: the project's own files
@pytest.mark.parametrize("kind,h,w,c,q", [("noise", 200, 333, 3, 95), ("impulses", 37, 53, 1, 30), (jpeg_cases.CROP, 64, 96, 3, 75), ("constant", 520, 24, 3, 95)])
def test_own_files_and_roundtrip(cuda_device, kind, h, w, c, q):
    """No restart markers, Annex K tables: the self-synchronising path on what a caller feeds back for the next iteration."""
    from neural_enhanced_super_resolution_amd import imgproc
    img, order = jpeg_cases.image(kind, h, w, c)
    frame = torch.from_numpy(np.ascontiguousarray(img)).to(cuda_device)
    data = imgproc.encode_jpeg_u8(frame, q, order=order)
    assert data == jpeg_cases.spec(kind, h, w, c, q)[0]
    want = ref.decode_jpeg(data, order)
    got = imgproc.decode_jpeg_u8(data, order=order, device=cuda_device, use_hip=True)
    assert np.array_equal(got.cpu().numpy(), want), _where(got.cpu().numpy(), want)
    again = imgproc.jpeg_roundtrip_u8(frame, quality=q, order=order)
    assert again.shape == frame.shape and torch.equal(again, got)
    if c == 1:
        assert torch.equal(imgproc.jpeg_roundtrip_u8(frame[:, :, None], quality=q)[:, :, 0], got)


# ------------------------------------------------------------------------------------------------ 10: enhance from a file
def _wrapper(device, **kw):
    from neural_enhanced_super_resolution_amd import RealESRGANer, RRDBNet
    from neural_enhanced_super_resolution_amd.synth import synthetic_state_dict
    sd = synthetic_state_dict(seed=3, num_in_ch=3, scale=2, num_block=2)
    return RealESRGANer(scale=2, model_path={"params_ema": sd}, model=RRDBNet(3, 3, scale=2, num_block=2), half=False, device=device, **kw)


@pytest.mark.parametrize("tile", [0, 32])
def test_enhance_file_equals_enhance_of_the_decoded_frame(cuda_device, tile, monkeypatch, tmp_path):
    from neural_enhanced_super_resolution_amd import realesrganer as R
    up = _wrapper(cuda_device, tile=tile, tile_pad=10, pre_pad=0)
    for c in (3, 1):
        data = dc.file_bytes(jpeg_cases.CROP, 64, 96, c, 2 if c == 3 else 0, 95, {})
        frame = np.ascontiguousarray(dc.spec_pixels(data, "bgr"))
        direct, mode = up.enhance(frame)
        uploads = []
        real = R.RealESRGANer._upload_u8
        monkeypatch.setattr(R.RealESRGANer, "_upload_u8", lambda self, img: uploads.append(type(img)) or real(self, img))
        got, fmode = up.enhance_file(data)
        monkeypatch.undo()
        assert fmode == mode == ("RGB" if c == 3 else "L")
        assert got.shape == direct.shape and got.std() > 0 and np.array_equal(got, direct)
        assert all(t is torch.Tensor for t in uploads) and (len(uploads) == 1 or c == 1), "the decoded frame must reach the route as a device tensor"
        assert np.array_equal(up.enhance(frame)[0], direct), "enhance() on ndarrays is unchanged"
        for kw in ({}, {"outscale": 1.5}):
            assert up.enhance_file_jpeg(data, **kw) == up.enhance_jpeg(frame, **kw)
            assert np.array_equal(up.enhance_file(data, **kw)[0], up.enhance(frame, **kw)[0])
    path = tmp_path / "crop.jpg"
    path.write_bytes(data)
    assert np.array_equal(up.enhance_file(str(path))[0], direct)
    for bad in (b"\x89PNG\r\n\x1a\n" + bytes(64), b""):
        with pytest.raises(ValueError, match="enhance_file"):
            up.enhance_file(bad)


def test_enhance_iterations_from_bytes(cuda_device):
    from neural_enhanced_super_resolution_amd import nesr_adapter as A
    data = dc.file_bytes("impulses", 24, 16, 3, 2, 95, {})
    cfg = {"iterations": 1, "upscale_factor": 2.0}
    want = A.enhance_iterations(None, np.ascontiguousarray(dc.spec_pixels(data)), cfg, device=cuda_device)
    assert np.array_equal(A.enhance_iterations(None, data, cfg, device=cuda_device), want)


# ------------------------------------------------------------------------------------------------ 11: rejected scans
def _rejected_files():
    plain = dc.file_bytes("noise", 40, 56, 3, 2, 95, {})
    marked = dc.file_bytes("noise", 40, 56, 3, 2, 95, {"restart_marker_blocks": 2})
    out = []
    for name, data in (("plain", plain), ("restart", marked)):
        start = ref.parse(data)["scan_offset"]
        middle = start + (len(data) - start) // 2
        out.append((name + "-cut", data[:middle]))
        noise = np.random.RandomState(11).randint(0, 256, len(data) - 2 - middle).astype(np.uint8).tobytes()
        out.append((name + "-noise", data[:middle] + noise + data[-2:]))
    at = marked.index(b"\xff\xd1", ref.parse(marked)["scan_offset"])
    out.append(("restart-number", marked[:at + 1] + b"\xd2" + marked[at + 2:]))
    return out, plain


def test_rejected_scans_end_in_the_status_word(cuda_device):
    """The bounds of the decode loops and the guards of the stores: a scan that breaks off, turns into noise or numbers its restart
    markers wrongly sets the status word (or decodes to the end), writes nothing outside the destination and the scratch, and
    leaves the next decode exact.  What libjpeg would recover from these files is not reproduced."""
    from neural_enhanced_super_resolution_amd import _lib, imgproc
    from neural_enhanced_super_resolution_amd._contexts import device_call
    lib = _lib.load()
    files, good = _rejected_files()
    for name, data in files:
        info = _lib.jpeg_parse(data)
        need = int(lib.nesr_jpeg_decode_scratch_bytes(ctypes.byref(info)))
        scratch = torch.full((need + 512,), 0xA5, dtype=torch.uint8, device=cuda_device)
        base = (-scratch.data_ptr()) % 256
        dst = torch.full((info.H + 2, info.W * 3 + 64), 0x5A, dtype=torch.uint8, device=cuda_device)
        status = torch.full((3,), 0x77777777, dtype=torch.int32, device=cuda_device)
        file_dev = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(cuda_device)
        device_call("nesr_jpeg_decode_u8", cuda_device, ctypes.c_void_p(file_dev.data_ptr()), len(data), ctypes.byref(info),
                    ctypes.c_void_p(dst[1:].data_ptr() + 32), dst.stride(0), 0, ctypes.c_void_p(scratch.data_ptr() + base), need,
                    ctypes.c_void_p(status[1:].data_ptr()))
        word = [int(v) & 0xFFFFFFFF for v in status.cpu()]
        assert word[0] == word[2] == 0x77777777, name
        s = scratch.cpu().numpy()
        assert (s[:base] == 0xA5).all() and (s[base + need:] == 0xA5).all(), name
        d = dst.cpu().numpy()
        assert (d[0] == 0x5A).all() and (d[-1] == 0x5A).all() and (d[:, :32] == 0x5A).all() and (d[:, 32 + info.W * 3:] == 0x5A).all(), name
        if word[1] == 0:
            assert tuple(imgproc.decode_jpeg_u8(data, device=cuda_device, use_hip=True).shape) == (info.H, info.W, 3), name
        else:
            with pytest.raises(_lib.NesrBadFileError) as e:
                imgproc.decode_jpeg_u8(data, device=cuda_device)
            assert e.value.status == word[1], name
        if name in ("plain-cut", "restart-cut", "restart-number"):
            assert word[1] != 0, name
        assert np.array_equal(imgproc.decode_jpeg_u8(good, device=cuda_device).cpu().numpy(), dc.spec_pixels(good)), f"the decode after {name}"


# ------------------------------------------------------------------------------------------------ 12: fallback
def test_unsupported_file_falls_back_to_pillow(cuda_device):
    pytest.importorskip("PIL")
    from PIL import Image
    from neural_enhanced_super_resolution_amd import _lib, imgproc
    buf = io.BytesIO()
    Image.fromarray(dc.image_rgb("impulses", 37, 53, 3)).save(buf, format="JPEG", quality=90, progressive=True)
    data = buf.getvalue()
    want = np.asarray(Image.open(io.BytesIO(data)))
    got = imgproc.decode_jpeg_u8(data, device=cuda_device)
    assert got.device.type == "cuda" and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(imgproc.decode_jpeg_u8(data, order="bgr", device=cuda_device).cpu().numpy(), want[:, :, ::-1])
    with pytest.raises(_lib.NesrUnsupportedError):
        imgproc.decode_jpeg_u8(data, device=cuda_device, use_hip=True)
    with pytest.raises(_lib.NesrBadFileError):
        imgproc.decode_jpeg_u8(data[:100], device=cuda_device)


# ------------------------------------------------------------------------------------------------ 13: the C host
def test_cpp_host_decodes_and_encodes(tmp_path, cuda_device):
    from neural_enhanced_super_resolution_amd import imgproc
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available on this box")
    exe = str(tmp_path / "jpeg_decode_host")
    subprocess.run([hipcc, "-O2", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "jpeg_decode_host.cpp"), "-o", exe, "-ldl"], check=True, timeout=300)
    lib = os.path.join(ROOT, "neural_enhanced_super_resolution_amd", "libnesr_hip.so")
    src = dc.golden_name(*dc.GOLDEN_FILES[6]) + ".jpg"
    dst = str(tmp_path / "out.jpg")
    out = subprocess.run([exe, lib, src, dst, "90"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    with open(src, "rb") as f:
        frame = imgproc.decode_jpeg_u8(f.read(), device=cuda_device, use_hip=True)
    with open(dst, "rb") as f:
        assert f.read() == imgproc.encode_jpeg_u8(frame, 90)

"""CPU: the host-side entries of the PNG encoder's C ABI (nesr_png_bound, nesr_png_scratch_bytes, nesr_png_head,
nesr_png_code_lengths, nesr_png_encode's argument checks) against the specification (tests/png_ref.py), and the host route of
imgproc.encode_png (cv2's settings restated with the standard library): the same pixels as the device route, different bytes."""
import ctypes
import io

import numpy as np
import pytest

from tests import png_cases, png_ref


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from neural_enhanced_super_resolution_amd import _lib
    return _lib.load()


def test_entries_are_declared_bound_and_exported(lib):
    from neural_enhanced_super_resolution_amd import _lib
    header = open(_lib.HERE + "/../include/nesr_hip.h").read()
    for name in ("nesr_png_bound", "nesr_png_scratch_bytes", "nesr_png_head", "nesr_png_code_lengths", "nesr_png_encode"):
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name)


def test_head_and_bound_equal_the_specification(lib):
    for h, w in ((1, 1), (37, 53), (32, 1023), (33, 1023), (2, 20000), (65535, 65535), (4320, 7680)):
        for c, depth in png_cases.KINDS:
            n = ctypes.c_int(-1)
            assert lib.nesr_png_head(h, w, c, depth, None, 0, ctypes.byref(n)) == 0 and n.value == 47        # the size alone
            buf = (ctypes.c_uint8 * 47)()
            assert lib.nesr_png_head(h, w, c, depth, buf, 47, ctypes.byref(n)) == 0
            assert bytes(buf) == png_ref.head(h, w, c, depth)
            assert lib.nesr_png_bound(h, w, c, depth) == png_ref.bound(h, w, c, depth)
            stream = h * (1 + w * c * depth // 8)
            assert lib.nesr_png_scratch_bytes(h, w, c, depth) >= stream + 32800 * ((stream + 32767) // 32768)
    assert lib.nesr_png_bound(0, 5, 3, 8) == 0 and lib.nesr_png_scratch_bytes(5, 5, 2, 8) == 0 and lib.nesr_png_bound(5, 5, 3, 12) == 0


def _lengths(lib, counts, limit):
    n = len(counts)
    arr = (ctypes.c_uint32 * n)(*[int(v) for v in counts])
    out = (ctypes.c_uint8 * n)()
    assert lib.nesr_png_code_lengths(arr, n, limit, out) == 0
    return list(out)


def _count_vectors(n, seed):
    rng = np.random.RandomState(seed)
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    yield [0] * n                                                   # nothing counted
    for s in (0, 1, n - 1):
        yield [7 if i == s else 0 for i in range(n)]                # one symbol
    yield [3 if i in (0, n - 1) else 0 for i in range(n)]           # two symbols
    yield [5 if i in (2, 3) else 0 for i in range(n)]
    k = min(n, 40)
    yield fib[:k] + [0] * (n - k)                                   # Fibonacci counts: depth k - 1, beyond 15 (and beyond 7)
    yield [0] * (n - k) + fib[:k][::-1]
    yield list(rng.permutation(fib[:k] + [0] * (n - k)))
    yield [1] * n                                                   # all equal: every tie
    while True:
        kind = rng.randint(0, 4)
        if kind == 0:
            v = rng.randint(0, 1000, n)
        elif kind == 1:
            v = rng.randint(0, 3, n) * rng.randint(1, 5, n)
        elif kind == 2:
            v = np.floor(np.exp(rng.uniform(0, 11, n))).astype(np.int64) * (rng.uniform(size=n) < 0.6)
        else:
            v = np.where(rng.uniform(size=n) < 0.1, rng.randint(1, 32768, n), 0)
        yield [int(x) for x in v]


# n in {286, 30, 19} x limit in {15, 7}: deflate's literal/length code, a distance code's size, the code-length code.  (286, 7) is
# left out: 286 symbols cannot all have codes of at most 7 bits, and the entry refuses the pair (test_code_lengths_refusals).
@pytest.mark.parametrize("n,limit", [(286, 15), (30, 15), (30, 7), (19, 15), (19, 7)])
def test_code_lengths_equal_the_specification(lib, n, limit):
    gen = _count_vectors(n, 1000 * n + limit)
    repaired = 0
    for _ in range(200):
        counts = next(gen)
        stats = {}
        want = png_ref.code_lengths(counts, limit, stats)
        got = _lengths(lib, counts, limit)
        assert got == want, counts
        repaired += len(stats)
        assert sum(2.0 ** -v for v in got if v) == 1.0, counts     # Kraft equality: a complete code
        assert max(got) <= limit and all((v > 0) or (c == 0) for v, c in zip(got, counts))
    assert repaired >= 3                                            # the repair rule ran (Fibonacci counts force it)


def test_code_lengths_refusals(lib):
    arr, out = (ctypes.c_uint32 * 286)(), (ctypes.c_uint8 * 286)()
    for args in ((None, 19, 7, out), (arr, 19, 7, None), (arr, 1, 7, out), (arr, 287, 15, out), (arr, 19, 0, out), (arr, 19, 16, out),
                 (arr, 286, 7, out)):
        assert lib.nesr_png_code_lengths(*args) == -1, args
    big = (ctypes.c_uint32 * 19)(*([0xFFFFFFFF] * 2 + [0] * 17))
    assert lib.nesr_png_code_lengths(big, 19, 7, out) == -1
    assert b"2^32" in lib.nesr_last_error()


def test_encode_refuses_bad_arguments_without_touching_a_device(lib):
    """Every NESR_ERR_ARG of nesr_png_encode; the pointers are never dereferenced (no device here)."""
    need = lib.nesr_png_scratch_bytes(37, 53, 3, 8)
    ok = dict(device=0, src=0x1000, stride=53 * 3, h=37, w=53, c=3, depth=8, order=0, scratch=0x2000, nscratch=need, out=0x3000, cap=100,
              words=0x4000, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.nesr_png_encode(a["device"], a["src"], a["stride"], a["h"], a["w"], a["c"], a["depth"], a["order"], a["scratch"], a["nscratch"],
                                   a["out"], a["cap"], a["words"], a["stream"])

    for bad in (dict(src=None), dict(scratch=None), dict(out=None), dict(words=None), dict(h=0), dict(w=0), dict(h=65536), dict(w=65536),
                dict(c=2), dict(c=5), dict(depth=12), dict(depth=1), dict(order=2), dict(order=-1), dict(stride=53 * 3 - 1),
                dict(depth=16, stride=53 * 6 - 1, nscratch=1 << 30), dict(nscratch=need - 1), dict(scratch=0x2008), dict(words=0x4004)):
        assert call(**bad) == -1, bad
        assert b"nesr_png_encode" in lib.nesr_last_error()


@pytest.mark.parametrize("kind", png_cases.KINDS, ids=[f"{c}x{d}" for c, d in png_cases.KINDS])
def test_host_route_decodes_to_the_frame(kind):
    import torch
    from neural_enhanced_super_resolution_amd import frame_io, imgproc
    c, depth = kind
    img = png_cases.content("impulses", 37, 53, c, depth)
    spec = png_cases.spec("impulses", 37, 53, c, depth)[0]
    for order in ("rgb", "bgr"):
        want = png_cases.file_order(img, order)
        data = imgproc.encode_png(img, order=order)                          # an ndarray: the host route
        got = png_ref.decode_png(data, layout=False)
        assert got.dtype == want.dtype and np.array_equal(got, want)
        assert imgproc.encode_png(frame_io.frame_to_tensor(img), order=order, use_hip=False) == data      # a CPU tensor (int16-held at 16 bit)
        if order == "rgb":
            assert data != spec and np.array_equal(png_ref.decode_png(spec), got)      # the same pixels, different bytes
    if c == 1:
        assert imgproc.encode_png(img[:, :, None]) == imgproc.encode_png(img)
    chunks = png_ref.read_chunks(imgproc.encode_png(img))
    assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    try:
        from PIL import Image
        if depth == 8 or c == 1:
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(imgproc.encode_png(img)))).astype(img.dtype), img)
    except ImportError:
        pass
    with pytest.raises(ValueError):
        imgproc.encode_png(img, order="rbg")
    with pytest.raises(ValueError):
        imgproc.encode_png(np.zeros((4, 4, 2), np.uint8))
    with pytest.raises(ValueError):
        imgproc.encode_png(np.zeros((4, 4, 3), np.float32))
    with pytest.raises(ValueError):
        imgproc.encode_png(torch.zeros(4, 4, 3, dtype=torch.uint8), use_hip=True)       # a CPU tensor cannot take the kernels

"""A numpy restatement, in plain loops, of the cv2 calls behind the rest of SuperResolutionPipeline.enhance_image's loop: one function
per cv2 (or numpy) call, named after it, each citing the reference line that makes the call.  The oracle of tests/test_stages_host.py;
it imports nothing of the product.  PARITY UNPINNED: cv2 is absent, so this restates OpenCV 4.x's published 8-bit arithmetic
(resize.cpp, morph, smooth, addWeighted) as the product does -- the tests compare two restatements written apart, and pin
restatement-free properties beside them.

Everything is uint8 HWC (or HW) ndarrays in, ndarrays out."""
import math

import numpy as np

INTER_NEAREST, INTER_LINEAR, INTER_CUBIC, INTER_LANCZOS4 = 0, 1, 2, 4
F = np.float32


def _position(n_in, n_out, d):
    """cv2.resize's sampling position of output d: (d + 0.5) scale - 0.5 in double, cast to float32; floor and fraction."""
    pos = F((d + 0.5) * (n_in / n_out) - 0.5)
    s = int(math.floor(pos))
    return s, F(pos - F(s))


def _short(v):
    """saturate_cast<short>(float): round half to even, saturate."""
    return int(min(max(np.rint(v), -32768), 32767))


def cubic_weights(f):
    """interpolateCubic (imgproc.hpp), A = -0.75, float32 throughout, left to right."""
    A, one = F(-0.75), F(1)
    f = F(f)
    x1 = F(f + one)
    w0 = F(F(F(F(F(F(A * x1) - F(F(5) * A)) * x1) + F(F(8) * A)) * x1) - F(F(4) * A))
    w1 = F(F(F(F(F(F(A + F(2)) * f) - F(A + F(3))) * f) * f) + one)
    g = F(one - f)
    w2 = F(F(F(F(F(F(A + F(2)) * g) - F(A + F(3))) * g) * g) + one)
    w3 = F(F(F(one - w0) - w1) - w2)
    return [w0, w1, w2, w3]


def axis_table(n_in, n_out, interp):
    """(first index, integer coefficients) per output position of one axis, as resize.cpp builds xofs / ialpha for 8-bit images."""
    first, coef = [], []
    for d in range(n_out):
        if interp == INTER_NEAREST:
            first.append(min(int(math.floor(d * (n_in / n_out))), n_in - 1))
            coef.append([1])
            continue
        s, f = _position(n_in, n_out, d)
        if interp == INTER_LINEAR:
            if s < 0:
                s, f = 0, F(0)
            if s >= n_in - 1:
                s, f = n_in - 1, F(0)
            first.append(s)
            coef.append([_short(F(F(1) - f) * F(2048)), _short(f * F(2048))])
        elif interp == INTER_CUBIC:
            first.append(s - 1)
            coef.append([_short(w * F(2048)) for w in cubic_weights(f)])
        else:
            raise ValueError(interp)
    return np.array(first, np.int64), np.array(coef, np.int64)


def resize(img, out_h, out_w, interp):
    """cv2.resize(img, (out_w, out_h), interpolation=interp) on uint8 HWC.
    nesr/nesr.py:601-605 (INTER_CUBIC, the no-model step), :732 (the default, INTER_LINEAR, on the object mask), :720-724
    (INTER_NEAREST on the class map); nesr/utils/image_utils.py:119-128 (downsample_image's INTER_CUBIC default)."""
    h, w, c = img.shape
    out = np.zeros((out_h, out_w, c), np.uint8)
    if interp == INTER_LINEAR and w == 2 * out_w and h == 2 * out_h:      # resize.cpp: INTER_LINEAR -> INTER_AREA at iscale 2 x 2
        for y in range(out_h):
            for x in range(out_w):
                for k in range(c):
                    blk = img[2 * y:2 * y + 2, 2 * x:2 * x + 2, k].astype(np.int64)
                    out[y, x, k] = (int(blk.sum()) + 2) >> 2
        return out
    xf, xa = axis_table(w, out_w, interp)
    yf, ya = axis_table(h, out_h, interp)
    if interp == INTER_NEAREST:
        for y in range(out_h):
            for x in range(out_w):
                out[y, x] = img[yf[y], xf[x]]
        return out
    taps = xa.shape[1]
    src = img.astype(np.int64)
    hor = np.zeros((h, out_w, c), np.int64)                               # HResize: integer sums
    for y in range(h):
        for x in range(out_w):
            for t in range(taps):
                sx = min(max(int(xf[x]) + t, 0), w - 1)
                hor[y, x] += src[y, sx] * int(xa[x, t])
    for y in range(out_h):
        rows = [min(max(int(yf[y]) + t, 0), h - 1) for t in range(taps)]
        for x in range(out_w):
            for k in range(c):
                if interp == INTER_LINEAR:                                # VResizeLinear<uchar, int, short>
                    b0, b1 = int(ya[y, 0]), int(ya[y, 1])
                    v = (((b0 * (int(hor[rows[0], x, k]) >> 4)) >> 16) + ((b1 * (int(hor[rows[1], x, k]) >> 4)) >> 16) + 2) >> 2
                else:                                                     # VResizeCubic + FixedPtCast<int, uchar, 22>
                    v = sum(int(ya[y, t]) * int(hor[rows[t], x, k]) for t in range(taps))
                    v = (v + (1 << 21)) >> 22
                out[y, x, k] = min(max(v, 0), 255)
    return out


def dilate3x3(mask):
    """cv2.dilate(mask, np.ones((3, 3), np.uint8), iterations=1) (nesr/nesr.py:735-736): the border value never wins the max."""
    h, w = mask.shape
    out = np.zeros_like(mask)
    for y in range(h):
        for x in range(w):
            out[y, x] = mask[max(y - 1, 0):min(y + 2, h), max(x - 1, 0):min(x + 2, w)].max()
    return out


def _reflect101(p, n):
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * (n - 1) - p
    return p


def gaussian_taps_sigma3():
    """getGaussianKernel for sigma 3, ksize round(6 sigma + 1) | 1 = 19, in OpenCV's 8-bit fixed point: x256, rounded, the centre
    making the sum 256."""
    k = [math.exp(-(i - 9) ** 2 / 18.0) for i in range(19)]
    tot = sum(k)
    q = [int(np.rint(v / tot * 256.0)) for v in k]
    q[9] += 256 - sum(q)
    return q


def gaussian_blur_sigma3(img):
    """cv2.GaussianBlur(img, (0, 0), 3) on uint8 HWC (nesr/nesr.py:739): separable fixed point, BORDER_REFLECT_101, (v + 2^15) >> 16."""
    h, w, c = img.shape
    q = gaussian_taps_sigma3()
    src = img.astype(np.int64)
    hor = np.zeros((h, w, c), np.int64)
    for y in range(h):
        for x in range(w):
            for t in range(19):
                hor[y, x] += q[t] * src[y, _reflect101(x + t - 9, w)]
    out = np.zeros((h, w, c), np.uint8)
    for y in range(h):
        for x in range(w):
            v = np.zeros(c, np.int64)
            for t in range(19):
                v += q[t] * hor[_reflect101(y + t - 9, h), x]
            out[y, x] = np.clip((v + (1 << 15)) >> 16, 0, 255)
    return out


def add_weighted_unsharp(img, blurred):
    """cv2.addWeighted(img, 1.5, blurred, -0.5, 0) (nesr/nesr.py:740): saturate_cast<uchar>(round half to even)."""
    v = np.rint(img.astype(np.float32) * F(1.5) - blurred.astype(np.float32) * F(0.5))
    return np.clip(v, 0, 255).astype(np.uint8)


def segment_and_enhance(img, seg_map):
    """_segment_and_enhance after the argmax (nesr/nesr.py:726-747) for a frame of at most 1024 pixels a side."""
    h, w = img.shape[:2]
    mask = (seg_map > 0).astype(np.uint8)                                                     # :731
    if mask.shape != (h, w):
        mask = resize(mask[:, :, None], h, w, INTER_LINEAR)[:, :, 0]                          # :732
    mask = dilate3x3(mask)                                                                    # :735-736
    sharpened = add_weighted_unsharp(img, gaussian_blur_sigma3(img))                          # :739-740
    return np.where(np.expand_dims(mask, 2) == 1, sharpened, img)                             # :743-747


def ensemble_mean(images):
    """nesr/nesr.py:1048-1054 on aligned images under NumPy 1.x: the float64 weight is cast to the array's float32, the product and
    the sum are float32, astype(np.uint8) truncates.  Written with explicit float32 scalars so that the NumPy at hand does not
    matter."""
    n = len(images)
    if n == 1:
        return images[0]
    wgt = F(1.0 / n)
    flat = [im.reshape(-1) for im in images]
    out = np.zeros(flat[0].shape, np.uint8)
    for i in range(flat[0].size):
        acc = F(0)
        for im in flat:
            acc = F(acc + F(F(im[i]) * wgt))
        out[i] = int(acc)
    return out.reshape(images[0].shape)


def ensemble_target(shapes):
    """nesr/nesr.py:1039: max over (h, w) tuples -- lexicographic."""
    return max([(s[0], s[1]) for s in shapes])

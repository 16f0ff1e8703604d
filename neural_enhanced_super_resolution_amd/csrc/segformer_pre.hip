// PIL's 8-bit resample (ImagingResample: Image.resize with BILINEAR or LANCZOS on an RGB image) as the SegFormer extractor of
// the reference uses it (nesr/nesr.py:709 and :712), one launch per pass: integer coefficients with 22 fractional bits, computed
// on the host in doubles (segformer_api.cpp), a uint8 image between the horizontal and the vertical pass.  The vertical pass can
// write the network's input instead: (v * (1 / 255) - mean) / std as NCHW float planes.
#include "segformer_api.h"

#include "nesr_kernels.h"

namespace nesr {
namespace {

__global__ __launch_bounds__(256) void seg_resample_kernel(const SegResample a) {
    const int ow = a.vertical ? a.w : a.out, oh = a.vertical ? a.out : a.h;
    const long long total = (long long)oh * ow * a.c;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int ch = (int)(idx % a.c);
    const long long px = idx / a.c;
    const int x = (int)(px % ow), y = (int)(px / ow);
    const int o = a.vertical ? y : x;
    const int lo = a.bounds[2 * o], n = a.bounds[2 * o + 1];
    const int* k = a.coef + (size_t)o * a.ksize;
    int acc = 1 << 21;
    if (a.vertical) {
        const uint8_t* p = a.src + ((size_t)lo * a.w + x) * a.c + ch;
        for (int j = 0; j < n; ++j) acc += (int)p[(size_t)j * a.w * a.c] * k[j];
    } else {
        const uint8_t* p = a.src + ((size_t)y * a.w + lo) * a.c + ch;
        for (int j = 0; j < n; ++j) acc += (int)p[(size_t)j * a.c] * k[j];
    }
    acc >>= 22;
    const int v = acc < 0 ? 0 : (acc > 255 ? 255 : acc);
    if (a.dst) a.dst[idx] = (uint8_t)v;
    if (a.dst_f32) {
        const float m = ch == 0 ? a.mean[0] : (ch == 1 ? a.mean[1] : (ch == 2 ? a.mean[2] : a.mean[3]));
        const float s = ch == 0 ? a.stdv[0] : (ch == 1 ? a.stdv[1] : (ch == 2 ? a.stdv[2] : a.stdv[3]));
        a.dst_f32[((size_t)ch * oh + y) * ow + x] = sub_rn(mul_rn((float)v, 1.0f / 255.0f), m) / s;
    }
}

}  // namespace

hipError_t launch_seg_resample(const SegResample& a, hipStream_t s) {
    if (a.h < 1 || a.w < 1 || a.c < 1 || a.c > 4 || a.out < 1 || a.ksize < 1) return hipErrorInvalidValue;
    const long long total = (long long)(a.vertical ? a.out : a.h) * (a.vertical ? a.w : a.out) * a.c;
    if (total > (1ll << 31) * 255) return hipErrorInvalidValue;
    seg_resample_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace nesr

// Single-launch entries of the UNet's fp16 kernels (nesr_unet_k_conv_f16, nesr_unet_k_rows_f16): test hooks as the nesr_unet_k_* of
// unet_kernel_api.cpp.  Each takes its f32 twin's arguments with the weight as the f16 packing unet_api.h documents, an optional
// range word and an optional place for the column block the launcher picked; fills the launcher's struct field for field and makes
// the one launch on the caller's stream.  No context, no allocation, no state.
#include "api_common.h"
#include "unet_api.h"

using namespace nesr;

namespace {

int done(hipError_t e, const char* entry, const char* launcher) { return launch_done(e, "csrc/unet_api.h", entry, launcher); }

UnetSrc source(const float* p, int c, int cs, const void* norm) { return UnetSrc{p, c, cs, static_cast<const VaeNorm*>(norm)}; }

}  // namespace

extern "C" {

int nesr_unet_k_conv_f16(int n, int H, int W, int stride, int up, const float* in0_dev, int c0, int cs0, const void* norm0_dev, const float* in1_dev, int c1,
                         int cs1, const void* norm1_dev, const void* w16_dev, const float* bias_dev, int cout, int coutp, const float* res_dev, int out_nchw,
                         float* out_dev, unsigned* range_dev, int* block_host, void* stream) {
    UnetConv16 a{};
    a.n = n, a.H = H, a.W = W, a.stride = stride, a.up = up;
    a.in[0] = source(in0_dev, c0, cs0, norm0_dev), a.in[1] = source(in1_dev, c1, cs1, norm1_dev);
    a.w16 = static_cast<const _Float16*>(w16_dev), a.status = range_dev;
    a.bias = bias_dev, a.cout = cout, a.coutp = coutp, a.res = res_dev, a.out_nchw = out_nchw, a.out = out_dev;
    const int rc = done(launch_unet_conv_f16(a, (hipStream_t)stream), "nesr_unet_k_conv_f16", "launch_unet_conv_f16");
    if (!rc && block_host) *block_host = unet_conv_f16_block(n, H, W, coutp);
    return rc;
}

int nesr_unet_k_rows_f16(int m, int rows_per_sample, const float* in0_dev, int c0, int cs0, const void* norm0_dev, const float* in1_dev, int c1, int cs1,
                         const void* norm1_dev, int prologue, const void* ln_dev, const float* ln_g_dev, const float* ln_b_dev, const void* w16_dev,
                         const float* b_dev, int ldw, int np, int geglu, const float* res_dev, float* out_dev, unsigned* range_dev, int* block_host,
                         void* stream) {
    UnetRows16 a{};
    a.m = m, a.rows_per_sample = rows_per_sample;
    a.in[0] = source(in0_dev, c0, cs0, norm0_dev), a.in[1] = source(in1_dev, c1, cs1, norm1_dev);
    a.prologue = prologue, a.ln = static_cast<const float4*>(ln_dev), a.ln_g = ln_g_dev, a.ln_b = ln_b_dev;
    a.w16 = static_cast<const _Float16*>(w16_dev), a.status = range_dev;
    a.b = b_dev, a.ldw = ldw, a.np = np, a.geglu = geglu, a.res = res_dev, a.out = out_dev;
    const int rc = done(launch_unet_rows_f16(a, (hipStream_t)stream), "nesr_unet_k_rows_f16", "launch_unet_rows_f16");
    if (!rc && block_host) *block_host = unet_rows_f16_block(m, np);
    return rc;
}

}  // extern "C"

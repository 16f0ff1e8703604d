// Internal interface of the SRVGGNetCompact path: the context entries of the C ABI (nesr_api.cpp) hand a context created by
// nesr_create_compact to compact_api.cpp, which drives the kernels of srvgg_compact.hip.  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nesr_kernels.h"

struct nesr_compact;

namespace nesr {

// ---- kernels (srvgg_compact.hip)
// operand form of a compact context: the 16-bit ones carry elem16.h's layout codes (E16<K>)
enum { COMPACT_SPLIT = 0, COMPACT_BF16 = 1, COMPACT_F16 = 3 };
struct CompactPack {
    const float* x;        // NCHW f32 [n][3][h][w], or null
    const uint8_t* u8;     // u8 HWC [h][w][3] (n == 1), or null
    int flip;              // u8: channel c of the network input is byte 2 - c
    int n, h, w;
    int form;              // destination form: COMPACT_SPLIT f32 NHWC [.][32], COMPACT_BF16 | COMPACT_F16 16-bit NHWC [.][32]
    void* out;             // the first conv's input, channels 3..31 zero
    float* res;            // f32 NHWC [.][4]: the image for the tail's residual
    unsigned* status;      // f16 form: sticky range word for the image it stages (may be null)
};
struct CompactConv {
    const void* in;        // NHWC activations: [n][h][w][cin] (bf16, f16 or f32)
    const void* wt;        // pack_compact_weights image
    const float* bias;     // [ncb * 16], zero padded
    const float* slope;    // [64]: activation slope for negative values (feature layers)
    void* out;             // NHWC [n][h][w][64] (feature layers)
    int n, h, w;
    unsigned* status;      // split and f16 forms: sticky range word (may be null)
};
hipError_t launch_compact_pack(const CompactPack& p, hipStream_t s);
hipError_t launch_compact_conv(const CompactConv& a, int form, int cin, int cus, hipStream_t s);
hipError_t launch_compact_tail(const CompactConv& a, int form, int scale, const float* res, float* y, uint8_t* y8, int flip, int round,
                               int cus, hipStream_t s);
size_t compact_weight_bytes(int cin_p, int ncb, int form);
void pack_compact_weights(const float* oihw, int cout, int cin, int cin_p, int ncb, int form, uint16_t* dst);

// ---- context (compact_api.cpp); the context entries of nesr_api.cpp hand a compact context on to these
int compact_create(nesr_compact** out, int device, int num_in_ch, int num_out_ch, int num_feat, int num_conv, int upscale, int act_type,
                   int dtype);
void compact_destroy(nesr_compact* c);
int compact_num_tensors(const nesr_compact* c);
int compact_upscale(const nesr_compact* c);   // output size / input size
int compact_load_weight(nesr_compact* c, const char* key, const float* data, const int64_t* shape, int ndim);
int compact_finalize(nesr_compact* c);
int compact_forward(nesr_compact* c, const float* x, const uint8_t* x_u8, int flip, int N, int C, int H, int W, float* y, uint8_t* y_u8,
                    int round_mode, hipStream_t s);
size_t compact_workspace_bytes(const nesr_compact* c, int N, int H, int W);
int compact_reserve(nesr_compact* c, int N, int H, int W);
double compact_flops(const nesr_compact* c, int N, int H, int W);
int compact_set_timing(nesr_compact* c, int enable);
int compact_kernel_time_ms(nesr_compact* c, double* total_ms, int64_t* launches, double* flops);
int compact_check_status(nesr_compact* c);
int compact_check_range(nesr_compact* c, hipStream_t s);

}  // namespace nesr

// Single-launch entries of the UNet's kernels (nesr_unet_k_*): test hooks for the per-launch parity tests, not pipeline entries.
// Each takes device pointers in the layout unet_api.h documents, fills the launcher's argument struct field for field and makes
// the one launch_unet_* call (the GroupNorm entry: a partial launch per source, then the finish) on the caller's stream.  No
// context, no allocation, no state: what a launcher refuses is NESR_ERR_ARG with nothing launched.
#include "api_common.h"
#include "unet_api.h"

using namespace nesr;

namespace {

int done(hipError_t e, const char* entry, const char* launcher) { return launch_done(e, "csrc/unet_api.h", entry, launcher); }

UnetSrc source(const float* p, int c, int cs, const void* norm) { return UnetSrc{p, c, cs, static_cast<const VaeNorm*>(norm)}; }

}  // namespace

extern "C" {

int nesr_unet_k_in(const float* src_dev, int nchw, int c, int cs, int m, long long rows, float* out_dev, void* stream) {
    UnetIn a{};
    a.src = src_dev, a.nchw = nchw, a.c = c, a.cs = cs, a.m = m, a.rows = rows, a.out = out_dev;
    return done(launch_unet_in(a, (hipStream_t)stream), "nesr_unet_k_in", "launch_unet_in");
}

int nesr_unet_k_embedding(double timestep, int c0, int td, int tdp, const float* w1_dev, const float* b1_dev, const float* w2_dev, const float* b2_dev,
                          const float* cls_dev, float* out_dev, void* stream) {
    UnetEmb a{};
    a.timestep = timestep, a.c0 = c0, a.td = td, a.tdp = tdp;
    a.w1 = w1_dev, a.b1 = b1_dev, a.w2 = w2_dev, a.b2 = b2_dev, a.cls = cls_dev, a.out = out_dev;
    return done(launch_unet_emb(a, (hipStream_t)stream), "nesr_unet_k_embedding", "launch_unet_emb");
}

int nesr_unet_k_temb(int count, int td, const float* semb_dev, const float* weights_dev, const unsigned long long* w_offset, const unsigned long long* b_offset,
                     const unsigned long long* cb_offset, const int* coutp, float* out_dev, void* stream) {
    if (count < 1 || count > UNET_MAX_RESNETS || !w_offset || !b_offset || !cb_offset || !coutp)
        return set_error(NESR_ERR_ARG, "nesr_unet_k_temb: count must be 1 .. " + std::to_string(UNET_MAX_RESNETS) + " with an offset triple and a coutp each; nothing was launched");
    UnetTemb a{};
    a.count = count, a.td = td, a.semb = semb_dev, a.weights = weights_dev, a.out = out_dev;
    for (int r = 0; r < count; ++r) a.r[r].w = w_offset[r], a.r[r].b = b_offset[r], a.r[r].cb = cb_offset[r], a.r[r].coutp = coutp[r];
    return done(launch_unet_temb(a, (hipStream_t)stream), "nesr_unet_k_temb", "launch_unet_temb");
}

int nesr_unet_k_conv(int n, int H, int W, int stride, int up, const float* in0_dev, int c0, int cs0, const void* norm0_dev, const float* in1_dev, int c1,
                     int cs1, const void* norm1_dev, const float* w_dev, const float* bias_dev, int cout, int coutp, const float* res_dev, int out_nchw,
                     float* out_dev, void* stream) {
    UnetConv a{};
    a.n = n, a.H = H, a.W = W, a.stride = stride, a.up = up;
    a.in[0] = source(in0_dev, c0, cs0, norm0_dev), a.in[1] = source(in1_dev, c1, cs1, norm1_dev);
    a.w = w_dev, a.bias = bias_dev, a.cout = cout, a.coutp = coutp, a.res = res_dev, a.out_nchw = out_nchw, a.out = out_dev;
    return done(launch_unet_conv(a, (hipStream_t)stream), "nesr_unet_k_conv", "launch_unet_conv");
}

int nesr_unet_k_group_norm(int n, int m, const float* in0_dev, int c0, int cs0, void* norm0_dev, double* partial0_dev, const float* in1_dev, int c1, int cs1,
                           void* norm1_dev, double* partial1_dev, int groups, const float* gamma_dev, const float* beta_dev, float eps, void* stream) {
    UnetGn a{};
    a.n = n, a.m = m, a.in[0] = source(in0_dev, c0, cs0, norm0_dev), a.in[1] = source(in1_dev, c1, cs1, norm1_dev);
    a.partial[0] = partial0_dev, a.partial[1] = partial1_dev, a.groups = groups, a.gamma = gamma_dev, a.beta = beta_dev, a.eps = eps;
    hipStream_t s = (hipStream_t)stream;
    int rc = done(launch_unet_gn_partial(a, 0, s), "nesr_unet_k_group_norm", "launch_unet_gn_partial");      // refuses before a launch what the finish would
    if (rc == NESR_OK && in1_dev) rc = done(launch_unet_gn_partial(a, 1, s), "nesr_unet_k_group_norm", "launch_unet_gn_partial");
    if (rc == NESR_OK) rc = done(launch_unet_gn_finish(a, s), "nesr_unet_k_group_norm", "launch_unet_gn_finish");
    return rc;
}

int nesr_unet_k_layer_norm_stats(const float* in_dev, int m, int c, int cs, float eps, void* out_dev, void* stream) {
    UnetLnStats a{};
    a.in = in_dev, a.m = m, a.c = c, a.cs = cs, a.eps = eps, a.out = static_cast<float4*>(out_dev);
    return done(launch_unet_ln_stats(a, (hipStream_t)stream), "nesr_unet_k_layer_norm_stats", "launch_unet_ln_stats");
}

int nesr_unet_k_rows(int m, int rows_per_sample, const float* in0_dev, int c0, int cs0, const void* norm0_dev, const float* in1_dev, int c1, int cs1,
                     const void* norm1_dev, int prologue, const void* ln_dev, const float* ln_g_dev, const float* ln_b_dev, const float* w_dev,
                     const float* b_dev, int ldw, int np, int geglu, const float* res_dev, float* out_dev, void* stream) {
    UnetRows a{};
    a.m = m, a.rows_per_sample = rows_per_sample;
    a.in[0] = source(in0_dev, c0, cs0, norm0_dev), a.in[1] = source(in1_dev, c1, cs1, norm1_dev);
    a.prologue = prologue, a.ln = static_cast<const float4*>(ln_dev), a.ln_g = ln_g_dev, a.ln_b = ln_b_dev;
    a.w = w_dev, a.b = b_dev, a.ldw = ldw, a.np = np, a.geglu = geglu, a.res = res_dev, a.out = out_dev;
    return done(launch_unet_rows(a, (hipStream_t)stream), "nesr_unet_k_rows", "launch_unet_rows");
}

int nesr_unet_k_attention(int samples, int nq, int nk, int heads, int d, const float* q_dev, const float* k_dev, const float* v_dev, int ldq, int ldkv, int ldo,
                          float* out_dev, void* stream) {
    UnetAttn a{};
    a.samples = samples, a.nq = nq, a.nk = nk, a.heads = heads, a.d = d, a.q = q_dev, a.k = k_dev, a.v = v_dev;
    a.ldq = ldq, a.ldkv = ldkv, a.ldo = ldo, a.out = out_dev;
    return done(launch_unet_attn(a, (hipStream_t)stream), "nesr_unet_k_attention", "launch_unet_attn");
}

}  // extern "C"

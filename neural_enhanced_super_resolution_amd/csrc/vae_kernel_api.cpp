// Single-launch entries of the VAE decoder's kernels (nesr_vae_k_*): test hooks for the per-launch parity tests, not pipeline
// entries.  Each takes device pointers in the layout vae_api.h documents, fills the launcher's argument struct field for field and
// makes the one launch_vae_* call (the GroupNorm entry: the partial launch, then the finish) on the caller's stream.  No context,
// no allocation, no state: what a launcher refuses is NESR_ERR_ARG with nothing launched.
#include "api_common.h"
#include "vae_api.h"

using namespace nesr;

namespace {

int done(hipError_t e, const char* entry, const char* launcher) { return launch_done(e, "csrc/vae_api.h", entry, launcher); }

}  // namespace

extern "C" {

int nesr_vae_k_in(const float* z_dev, int c, int m, float divisor, float* out_dev, void* stream) {
    VaeIn a{};
    a.z = z_dev, a.c = c, a.m = m, a.divisor = divisor, a.out = out_dev;
    return done(launch_vae_in(a, (hipStream_t)stream), "nesr_vae_k_in", "launch_vae_in");
}

int nesr_vae_k_conv(int in_mode, const float* in_dev, int H, int W, int cin, int cinp, int cs_in, const void* norm_dev, const float* w_dev,
                    const float* bias_dev, int cout, int coutp, const float* res_dev, int cs_res, int out_mode, void* out_dev, int cs_out, void* stream) {
    VaeConv a{};
    a.in_mode = in_mode, a.in = in_dev, a.H = H, a.W = W, a.cin = cin, a.cinp = cinp, a.cs_in = cs_in;
    a.norm = static_cast<const VaeNorm*>(norm_dev), a.w = w_dev, a.bias = bias_dev, a.cout = cout, a.coutp = coutp;
    a.res = res_dev, a.cs_res = cs_res, a.out_mode = out_mode, a.out = out_dev, a.cs_out = cs_out;
    return done(launch_vae_conv(a, (hipStream_t)stream), "nesr_vae_k_conv", "launch_vae_conv");
}

int nesr_vae_k_group_norm(const float* in_dev, int m, int c, int cs, int groups, double* partial_dev, const float* gamma_dev, const float* beta_dev,
                          float eps, void* norm_dev, void* stream) {
    VaeStats a{};
    a.in = in_dev, a.m = m, a.c = c, a.cs = cs, a.groups = groups, a.partial = partial_dev;
    a.gamma = gamma_dev, a.beta = beta_dev, a.eps = eps, a.out = static_cast<VaeNorm*>(norm_dev);
    hipStream_t s = (hipStream_t)stream;
    int rc = done(launch_vae_stats_partial(a, s), "nesr_vae_k_group_norm", "launch_vae_stats_partial");      // refuses before a launch what the finish would
    if (rc == NESR_OK) rc = done(launch_vae_stats_finish(a, s), "nesr_vae_k_group_norm", "launch_vae_stats_finish");
    return rc;
}

int nesr_vae_k_rows(int m, int cs_in, int np, const float* in_dev, const void* norm_dev, const float* w_dev, const float* b_dev, const float* res_dev,
                    float* out_dev, void* stream) {
    VaeRows a{};
    a.m = m, a.cs_in = cs_in, a.np = np, a.in = in_dev, a.norm = static_cast<const VaeNorm*>(norm_dev);
    a.w = w_dev, a.b = b_dev, a.res = res_dev, a.out = out_dev;
    return done(launch_vae_rows(a, (hipStream_t)stream), "nesr_vae_k_rows", "launch_vae_rows");
}

int nesr_vae_k_attention(int n, int c, int cs, const float* qkv_dev, float* out_dev, void* stream) {
    VaeAttn a{};
    a.n = n, a.c = c, a.cs = cs, a.qkv = qkv_dev, a.out = out_dev;
    return done(launch_vae_attn(a, (hipStream_t)stream), "nesr_vae_k_attention", "launch_vae_attn");
}

}  // extern "C"

// The RRDBNet context behind the C ABI: what a compute form is (Form), the context itself (nesr_ctx) and the stages of its
// forward graph (rrdb_forward.cpp).  Shared by nesr_api.cpp, band_api.cpp, shard_api.cpp and oneshot_api.cpp; not part of the
// public ABI (that is include/nesr_hip.h).
#pragma once
#include <string>
#include <unordered_map>
#include <vector>

#include "api_common.h"
#include "compact_api.h"
#include "nesr_kernels.h"

namespace nesr {

// One compute form (NESR_DTYPE_*): everything the host code needs to know about it, in one row of FORMS (rrdb_forward.cpp).
struct Form {
    int kind;        // activation layout / kernel family: 0 f32 NHWC, 1 bf16 blocked, 2 f16 hi|lo blocked, 3 f16 blocked (PackArgs::bf16)
    int esize;       // bytes per stored activation value
    int kgroup;      // K-group of the conv kernel: cin padding granule
    size_t (*weight_elems)(int cin_p, int coutp);   // packed weight slab of one layer, in units of ...
    int weight_unit;                                // ... this many bytes
    void (*pack)(const float* oihw, int cout, int cin, int cin_p, int coutp, void* dst);
    hipError_t (*launch)(const ConvArgs& a, hipStream_t s);   // one 3x3 conv per launch
    bool ranged;     // has a range word: a stored value beyond +-65504 turns the output into NaN (NESR_ERR_RANGE)

    size_t weight_bytes(int cin_p, int coutp) const { return weight_elems(cin_p, coutp) * weight_unit; }
};
const Form* form_of(int dtype);   // null: not a NESR_DTYPE_*

// kind 0 (f32): NHWC (pix = channels of the buffer, chunk = 8).  kind 1 (bf16), kind 3 (f16): channel-blocked
// [C/16][pixels][16].  kind 2 (f16 pairs): [C/16][pixels][16 hi | 16 lo], in 2-byte units.
Map make_map(int kind, int channels, size_t pixels);

struct Layer {
    std::string name;
    int cin = 0, cout = 0, cin_p = 0, cout_p = 0;
    std::vector<float> w, b;  // host copies until finalize
    bool has_w = false, has_b = false;
    void* d_w = nullptr;
    void* d_ww = nullptr;   // Winograd-transformed weights (f32 Winograd contexts)
    void* d_w2 = nullptr;   // conv_up1 / conv_up2 of f16-pair contexts: the four folded 2x2-tap slabs (upconv2x2_f16x2.hip)
    float* d_b = nullptr;
};

// byte offsets of the feature maps inside the workspace
struct WsLayout {
    size_t in, f, a, b, c, u1, u2, u3, sync, total;
    int sync_words;
};
// geometry + workspace views of one evaluation (see fw_* below)
struct FwState {
    int N = 0, h = 0, w = 0;      // batch, internal (trunk) height and width
    WsLayout L;
    Map m_in, m_f, m_t, m_u1, m_u2;
    char* buf[3] = {nullptr, nullptr, nullptr};
};

// Row bands of one frame on several contexts of ONE process (band_api.cpp): the neighbours of a context, the landing buffers
// their band_push_edges launches write into, and what the whole-frame driver (nesr_forward_banded*) keeps between frames.
constexpr int BAND_APRON = 6;        // banded.APRON: internal rows of each neighbour a band carries
struct BandLink {
    nesr_ctx* nb[2] = {nullptr, nullptr};        // [0] the band above, [1] the band below
    bool direct[2] = {false, false};             // the link to nb[i] is written by the push kernel (same device, or peer access); false: staged copy
    bool force_staged = false;                   // nesr_band_set_staged: every link of this context is staged
    char* land[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};   // [side the rows come from][step parity], BAND_APRON rows each; owned by the RECEIVER
    size_t land_bytes = 0;                       // of each landing buffer
    char* send[2] = {nullptr, nullptr};          // staged links: the packed rows going up / down
    size_t send_bytes = 0;
    hipEvent_t pushed[2] = {nullptr, nullptr};   // [step parity] behind this context's push of that step
    hipEvent_t start = nullptr, done = nullptr;  // frame driver: behind the frame's input on the first band's stream; behind a band's output copy
    hipStream_t stream = nullptr;                // frame driver: the band's stream when the caller gives none
    char* io[2] = {nullptr, nullptr};            // frame driver: the band's input rows / its output image, on this context's device
    size_t io_bytes[2] = {0, 0};
};

}  // namespace nesr

struct nesr_ctx {
    nesr_compact* compact = nullptr;   // nesr_create_compact: an SRVGGNetCompact context (compact_api.cpp); no other field is used
    int device = 0, cin0 = 3, unshuffle = 0, nf = 64, nb = 23, gc = 32, nout = 3, dtype = 0;
    const nesr::Form* form = nullptr;   // the row of `dtype`
    bool winograd = false;   // f32 feature-map convs by Winograd F(2x2,3x3) (NESR_DTYPE_F32_WINOGRAD; stored as dtype F32)
    std::vector<nesr::Layer> layers;
    std::unordered_map<std::string, int> index;
    bool finalized = false;
    char* d_weights = nullptr;   // arena: [256 B of zeros | packed weights and biases]
    char* ws = nullptr;
    size_t ws_bytes = 0;
    nesr::TrunkLayer* d_trunk = nullptr;   // device copy of the trunk's layer table (persistent trunk kernel)
    unsigned* last_sync = nullptr;   // abort word of the most recent persistent trunk launch
    int trunk_mode = 0;              // 0 auto, 1 per-layer launches, 2 persistent kernel
    int shared_device = 0;           // nesr_set_concurrent: other contexts run on the device at the same time
    int size_independent = 0;        // nesr_set_size_independent: kernel choice must not depend on the image size
    int last_narrow = 1;             // nesr_set_conv_last / NESR_CONV_LAST: conv_last of the f16-pair form as one 16-channel column block
    int upconv_2x2 = 1;              // nesr_set_upconv / NESR_UPCONV: the nearest-x2 convs as four 2x2-tap convs (f16-pair form); 0: 3x3
    // the ragged batch being evaluated (nesr_forward_ragged): internal-resolution sizes of its images
    int rag_n = 0, rag_base_h = 0;
    unsigned short rag_h[nesr::RAG_MAX], rag_w[nesr::RAG_MAX];
    unsigned* d_status = nullptr;    // [0] sticky range word of the f16-pair path (ConvArgs::status), [1] abort word of the fused
                                     // dense-block kernel, [64..] its per-tile progress words
    unsigned rdb_epoch = 0;          // fused dense-block launches: progress values of a launch are epoch+1 .. epoch+4
    int rdb_mode = -1;               // NESR_RDB_FUSE: -1 auto (fuse when every tile gets its own CU), 0 never
    int rdb_chain = 1;               // NESR_RDB_CHAIN: 1 the trunk's dense blocks as one chained launch where the fused kernel applies, 0 one launch per block
    nesr::RdbChainBlock* d_chain = nullptr;       // the chained launch's per-block pointers ...
    std::vector<nesr::RdbChainBlock> h_chain;     // ... and what they were built from (rebuilt when workspace or weights have moved)
    int chain_launches = 0, chain_blocks = 0;     // the last forward's fused f32 dense blocks: kernel launches, blocks (nesr_rdb_chain_state)
    int cus = 256;
    unsigned* h_status = nullptr;    // pinned landing word of nesr_check_range
    // bf16 dense blocks with the working set resident in LDS (rdb_bf16_strip.hip)
    char* d_strip = nullptr;         // per dense block: weight stream (strip_weight_bytes()) + 192 f32 of bias
    size_t strip_stride = 0;
    int strip_mode = -1;             // NESR_STRIP: -1 auto (size-independent contexts, or batches that fill the device), 0 never, 1 wherever it applies
    unsigned strip_epoch = 0;
    bool strip_used = false;         // a strip launch went out since the last status check
    unsigned long long strip_timeout_ticks = 20000000ull;   // 200 ms of s_memrealtime: what an inter-workgroup wait of a persistent kernel may take
    int rdb_mode_init = -1, strip_mode_init = -1;
    int strip_seg = 0;               // NESR_STRIP_SEG: positions per row segment of a strip at most (0: the packer decides, -1: never cut)
    int strip_cus = 0;               // NESR_STRIP_CUS: the workgroups the packer plans for, 1 .. cus (0: cus)
    // sharded frames (nesr_comm_init / nesr_forward_sharded_u8): RCCL communicator + scratch
    void* comm = nullptr;            // ncclComm_t
    int comm_rank = 0, comm_nranks = 1;
    char* shard_buf = nullptr;
    size_t shard_bytes = 0;
    int debug_drop = 0;              // nesr_debug_fault: workgroups the next persistent launch leaves out
    int fused_aborts = 0;            // persistent launches that gave up (the context runs per-layer launches from then on)
    struct StripPlan {
        std::vector<int> key;        // N, H, W, then (h, w) of every image
        void* d_items = nullptr; int* d_first = nullptr; char* d_xch = nullptr;
        int grid = 0, smax = 0, makespan = 0;
        double efficiency = 0.0;
    };
    std::vector<StripPlan> strip_plans;
    nesr::FwState band;              // the banded evaluation in progress (nesr_band_*)
    bool band_valid = false;
    nesr::BandLink link;             // row bands inside one process (nesr_band_link, nesr_forward_banded*)
    nesr::EventTimer timer;          // kernel timing hook

    size_t esize() const { return form->esize; }
    int kind() const { return form->kind; }
    bool ranged() const { return form->ranged; }
    // the 16-bit forms (bf16, f16): the same kernels, layouts, strip plans, leases and ragged batches
    bool half16() const { return dtype == NESR_DTYPE_BF16 || dtype == NESR_DTYPE_F16; }
    int ct() const { return nf + 4 * gc; }  // channels of a dense-block buffer
    int ufac() const { return unshuffle > 1 ? unshuffle : 1; }
};

namespace nesr {

// The guard of the entries that exist for RRDBNet alone: NESR_ERR_ARG with the entry's name in the text for a compact context,
// NESR_OK for any other pointer, null included (what a null context gets differs per entry)
int rrdb_only(const nesr_ctx* c, const char* entry);
#define RRDB_ONLY(c)                                                  \
    do {                                                              \
        if (int rc__ = nesr::rrdb_only((c), __func__)) return rc__;   \
    } while (0)

inline int layer_id(int b, int r, int k) { return 1 + (b * 3 + r) * 5 + k; }  // RDB r, conv k of RRDB b; r, k zero based
inline double conv_flops(const Layer& L, double pixels) { return 2.0 * 9.0 * L.cin * L.cout * pixels; }

// ---- band_api.cpp: nesr_destroy's part of the band links (neighbours forget `c`; buffers, events and stream are freed)
void band_release(nesr_ctx* c);

// ---- rrdb_forward.cpp
// dense block r of RRDB b: the rotation of the three trunk buffers and the block's weights (the fused routes' arguments)
void rdb_block_entry(char* const buf[3], const Layer* layers, int b, int r, RdbChainBlock& e);
WsLayout ws_layout(const nesr_ctx* c, int N, int h, int w);
int ensure_ws(nesr_ctx* c, size_t bytes);
void free_strip_plans(nesr_ctx* c);
void lease_forget(const nesr_ctx* c);
// the forward graph in stages (whole-frame forward = all of them in order; the banded multi-GPU mode runs them one at a
// time with a row exchange in between)
int fw_setup(nesr_ctx* c, int N, int C, int H, int W, FwState& F);
int fw_first(nesr_ctx* c, const FwState& F, const float* x_f32, const uint8_t* x_u8, int flip, int C, int H, int W, hipStream_t s,
             const Pack12Args* nesr12 = nullptr);
int fw_rdb(nesr_ctx* c, const FwState& F, int b, int r, hipStream_t s, int phase = -1, int top = 0, int bottom = 0, int edge = 0);
int fw_tail(nesr_ctx* c, const FwState& F, float* y_f32, uint8_t* y_u8, int flip, int round_mode, hipStream_t s);
// The whole forward.  x -> y; exactly one of (x_f32, x_u8, nesr12) and one of (y_f32, y_u8) is set.  nesr12: the input is the
// 12-channel synthesis of that window (nesr12.hip; its destination fields are filled here), N = 1, C = 12, H x W the window.
// y_u8_row_bytes: bytes between the rows of y_u8 (0: contiguous rows).
int run_forward(nesr_ctx* c, const float* x_f32, const uint8_t* x_u8, int flip, int N, int C, int H, int W,
                float* y_f32, uint8_t* y_u8, int round_mode, hipStream_t s, const Pack12Args* nesr12 = nullptr, long long y_u8_row_bytes = 0);

}  // namespace nesr

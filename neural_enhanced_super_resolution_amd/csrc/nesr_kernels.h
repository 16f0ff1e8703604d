// Internal launcher interface between the C-ABI layer (rrdb_ctx.h: the table of compute forms and the files it lists) and the HIP kernels.
// Not part of the public ABI (that is include/nesr_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>
#include <vector>

namespace nesr {

// Single-precision operations that round by themselves, for kernels that restate a chain of torch operations bit for bit
// (imgproc.hip, filters.hip): hipcc contracts a * b + c into an fma also when it is spelled __fadd_rn(__fmul_rn(a, b), c) (and
// `#pragma clang fp contract(off)` does not reach those intrinsics); the torch operations are separate kernels and never do.
__device__ __forceinline__ float mul_rn(float a, float b) { float r; asm("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float add_rn(float a, float b) { float r; asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float sub_rn(float a, float b) { float r; asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }

// v * s + q in TWO roundings, as the residuals of every compute form are specified (tests/pair_spec.py holds the f16-pair
// kernels to it per value, tests/rdb16_block.py the bf16 / f16 ones).  __fmul_rn / __fadd_rn do not give that here: the
// toolchain's headers define them as plain * and +, which hipcc's default -ffp-contract=fast fuses into one v_(pk_)fma_f32.
// The pragma takes the contraction off these two operations alone.
__device__ __forceinline__ float scale_add_2r(float v, float s, float q) {
#pragma clang fp contract(off)
    const float p = v * s;
    return p + q;
}

// XCD-aware work index of this workgroup among `total` (bijective for any count): consecutive workgroup ids go round the
// 8 XCDs, so XCD x takes the contiguous range of work items that starts at x's share -- neighbours in the work order
// (a tile's cout groups, adjacent tiles) share an L2.
__device__ __forceinline__ int xcd_work_index(int total) {
    const int bid = blockIdx.x, q = total >> 3, r = total & 7, xcd = bid & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}

// Activation addressing.  Channels are grouped in K-groups of KG channels (8 for f32, 16 for
// bf16 = 32 bytes, one MFMA K-chunk); element (pixel p, channel c) of a feature map lives at
//     base + (c / KG) * chunk + p * pix + (c % KG)          (in elements)
//   NHWC (f32 path)            : pix = C_total, chunk = KG      -> base + p*C + c
//   channel-blocked (bf16 path): pix = KG,      chunk = P*KG    -> [C/KG][P pixels][KG]
// The blocked form makes one K-chunk of neighbouring pixels contiguous in HBM, so the staging
// loads / LDS-DMA read whole 128-byte lines (NHWC gives every lane its own line: the bf16 kernels
// were L1-access-bound, profiles/r01/bf16_tcp_bound.txt).  SURVEY.md section 7's "one 192-channel
// buffer whose channel slices are x0|x1|x2|x3|x4" holds in both forms: a slice is a channel range.
struct Map {
    int pix;          // elements between consecutive pixels
    long long chunk;  // elements between consecutive K-groups
};

// More than 64 KiB of dynamic LDS needs an opt-in per kernel AND per device: a process may hold contexts on
// several GPUs (nesr_create's device_id), and the attribute belongs to the device's copy of the code object.
// `done` is the launcher's static bitmask of devices already set (a benign race: the call is idempotent).
inline hipError_t ensure_dynamic_lds(const void* kernel, size_t bytes, unsigned long long& done) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 64 && ((done >> dev) & 1ull)) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess && dev < 64) done |= 1ull << dev;
    return e;
}

constexpr int RAG_MAX = 64;   // images per ragged batch

// One fused 3x3 / stride 1 / zero-pad 1 convolution (torch.cat-free dense block: conv k reads
// channels [0, cin) and writes channels [out_coff, out_coff + coutp) of the same buffer).
struct ConvArgs {
    // input: channels [0, cin) are read
    const void* in;
    Map in_map;
    int in_h, in_w;        // stored (source) height/width
    int up;                // 1: the logical input is the nearest x2 upsample of the stored one
                           //    (F.interpolate(scale_factor=2, mode='nearest') folded into addressing)
    int cin;               // padded to a multiple of KG
    // packed weights / bias (device)
    const void* w;
    const float* bias;     // [coutp] f32
    int coutp;             // padded output channels: 32 or 64
    // geometry of the convolution (logical input == output spatial size)
    int n, h, w_;
    // output rows [y_lo, y_hi) only (0, 0 = all of [0, h)): the banded multi-GPU mode computes the rows its neighbours
    // wait for first.  The input is still the whole image: rows outside [0, h) are the zero padding, rows outside
    // [y_lo, y_hi) are real data.  conv3x3_f16x2_kernel only (the other launchers reject a row range).
    int y_lo, y_hi;
    // feature-map output (may be null when out_nchw / out_u8 is used)
    void* out;
    Map out_map;
    int out_coff;
    void* out2;            // optional second copy of the same values (channels [0,coutp))
    Map out2_map;
    // epilogue: v = acc + bias; if lrelu v = leaky(v, 0.2); if res1 v = v*s1 + res1; if res2 v = v*s2 + res2
    int lrelu;
    const void* res1; Map res1_map; float s1;
    const void* res2; Map res2_map; float s2;
    // planar f32 output [n][cout_real][h][w] (conv_last feeding RRDBNet.forward's NCHW result)
    float* out_nchw;
    int cout_real;
    // fused image output: u8 HWC [h][w][3], clamp(0,1) * 255, optional channel flip
    uint8_t* out_u8;
    int u8_flip, u8_round;
    // >= 16 bytes of device zeros: LDS-DMA source for out-of-image pixels (bf16 large-tile kernel)
    const void* zeros;
    // f16-pair path: sticky device word set when a value does not fit the (hi, lo) pair (|x| > 65504 or not
    // finite); conv_last reads it and writes NaN instead of a saturated image.  May be null.
    unsigned* status;
    // host-side hint, not read by kernels: other contexts' launches share the device with this one (frames or tile
    // groups in flight on several streams) -- prefer kernel forms whose workgroups leave room on a CU
    int shared_device;
    // Images of different sizes in one batch (nesr_forward_ragged: the tiles of a frame, whose edge tiles are smaller):
    // image i occupies the top-left (rag_h[i] << rag_shift) x (rag_w[i] << rag_shift) pixels of its h x w slot, the rest
    // of the slot is neither read (it counts as the zero padding) nor written.  rag_n = 0: every image is h x w.  The
    // sizes travel in the kernel arguments (no device table, no copy to order).  conv3x3_bf16_xl_kernel only.
    int rag_n, rag_shift;
    // host-side hint: choose the kernel by arithmetic only, never by image size (nesr_set_size_independent): a tile's bits
    // must not depend on whether it was evaluated alone or inside a ragged batch
    int size_independent;
    // host-side: conv_last of the f16-pair form (image outputs only, cout_real <= 4) computes one 16-channel MFMA column block
    // instead of the cout group's two -- a scheduling change, bit-identical output (conv3x3_f16x2_kernel<DMAW, 1>)
    int narrow_last;
    unsigned short rag_h[RAG_MAX], rag_w[RAG_MAX];
};

// Which kernel family a conv launcher chose (NESR_CONV_KERNEL_* of include/nesr_hip.h): every launcher below notes it at the
// point of dispatch, per host thread; nesr_debug_last_conv_kernel reports what the single-layer hooks' launch noted
// (oneshot_api.cpp).  A thread-local store: nothing on the device, nothing a forward waits for.
enum { CONV_KERNEL_NONE = 0, CONV_KERNEL_GENERIC = 1, CONV_KERNEL_XL = 2, CONV_KERNEL_WINOGRAD = 3, CONV_KERNEL_F16_PAIR = 4, CONV_KERNEL_UPCONV2X2 = 5 };
void note_conv_kernel(int family);

// f32 path: v_mfma_f32_32x32x2_f32 implicit GEMM (conv3x3_mfma.hip)
hipError_t launch_conv3x3_f32(const ConvArgs& a, hipStream_t s);
// host-side weight repack for the f32 kernel: OIHW f32 -> [cin/8][tap][half][coutp][4]
size_t packed_weight_elems_f32(int cin_p, int coutp);
void pack_weights_f32(const float* oihw, int cout, int cin, int cin_p, int coutp, float* dst);

// f32 Winograd F(2x2,3x3) path: v_mfma_f32_16x16x4_f32, 2.25x less matrix work (conv3x3_wino_f32.hip);
// feature-map outputs only (conv_last keeps the direct kernel)
hipError_t launch_conv3x3_wino_f32(const ConvArgs& a, hipStream_t s);
size_t packed_weight_elems_wino_f32(int cin_p, int coutp);
void pack_weights_wino_f32(const float* oihw, int cout, int cin, int cin_p, int coutp, float* dst);

// bf16 path: v_mfma_f32_32x32x16_bf16 implicit GEMM (conv3x3_bf16.hip)
hipError_t launch_conv3x3_bf16(const ConvArgs& a, hipStream_t s);       // picks the variant by frame size
const char* bad_kernel16_override();   // the value of NESR_BF16_KERNEL if it is neither small nor xl (callers refuse it by name), else null
hipError_t launch_conv3x3_bf16_xl(const ConvArgs& a, hipStream_t s);    // conv3x3_bf16.hip: 16x32-px tiles (NESR_XL_GEOMETRY=8: 32x32), LDS-DMA ring
size_t packed_weight_elems_bf16(int cin_p, int coutp);
void pack_weights_bf16(const float* oihw, int cout, int cin, int cin_p, int coutp, uint16_t* dst);
// f16 path: the same kernels instantiated on f16 (v_mfma_f32_32x32x16_f16), the same layouts; every stored activation is
// range-checked (|x| <= 65504, finite) into ConvArgs::status, and conv_last writes NaN once that word is set
hipError_t launch_conv3x3_f16(const ConvArgs& a, hipStream_t s);        // picks the variant as launch_conv3x3_bf16 does
hipError_t launch_conv3x3_f16_xl(const ConvArgs& a, hipStream_t s);
void pack_weights_f16(const float* oihw, int cout, int cin, int cin_p, int coutp, uint16_t* dst);   // packed_weight_elems_bf16 elements

// f32 path on the f16 matrix cores (conv3x3_f16x2.hip): operands as (hi, lo) half pairs, x = hi + lo * 2^-11,
// three MFMAs per product, f32 accumulation.  Activations: channel-blocked [C/16][pixels][16 hi | 16 lo]
// (Map in 2-byte units: pix = 32, chunk = pixels * 32).
hipError_t launch_conv3x3_f16x2(const ConvArgs& a, hipStream_t s);
size_t packed_weight_elems_f16x2(int cin_p, int coutp);   // in 2-byte units
void pack_weights_f16x2(const float* oihw, int cout, int cin, int cin_p, int coutp, uint16_t* dst);

// conv3x3(nearest_x2(x)) as four 2x2-tap convs on the stored (low-res) input, f16-pair form (upconv2x2_f16x2.hip): a.up = 1,
// a.h = 2 a.in_h, a.w_ = 2 a.in_w, a.w = pack_upconv_weights_f16x2's image; feature-map output only, whole images.
// fold_upconv_weights: OIHW f32 [cout][cin][3][3] -> [py][px][a][b][cout][cin] f32 (16 cout cin values), the taps that read
// low-res pixel (y + py - 1 + a, x + px - 1 + b) at output parity (py, px) summed in f32, ky ascending, then kx.
hipError_t launch_upconv2x2_f16x2(const ConvArgs& a, hipStream_t s);
void fold_upconv_weights(const float* oihw, int cout, int cin, float* dst);
size_t packed_upconv_elems_f16x2(int cin_p, int coutp);   // in 2-byte units
void pack_upconv_weights_f16x2(const float* folded, int cout, int cin, int cin_p, int coutp, uint16_t* dst);

// One residual dense block (conv1..conv5) per launch, f16-pair form, for frames whose 8x32-pixel tiles all get their
// own resident workgroup (rdb_f16x2.hip, rdb_f16x2_kernel): tiles = rdb_f16x2_tiles(n, h, w) <= compute units.
struct RdbLaunch {
    const void* cur;          // the block's 192-channel buffer (f16-pair layout: [12 chunks][pixels][64 B])
    long long chunk_bytes;
    void* out;                // conv5 destination buffer (its channels 0..63)
    const void* res2;         // RRDB input for the second residual, or null
    float s1, s2;
    const void* w[5];
    const float* bias[5];
    int n, h, w_;
    unsigned* progress;       // [tiles] device words, monotonic across launches
    unsigned epoch;           // strictly increasing by >= 8 per launch
    unsigned* abort_flag;
    unsigned* status;
    unsigned long long timeout_ticks;   // 100 MHz ticks a neighbour wait may take (0: 200 ms)
    int debug_drop;           // test hook: this many workgroups of the launch never start
};
int rdb_f16x2_tiles(int n, int h, int w);
hipError_t launch_rdb_f16x2(const RdbLaunch& r, hipStream_t s);
// A run of consecutive dense blocks of one forward in one launch (rdb_f16x2_chain_kernel): what differs from block to block,
// one entry per block in device memory.  r.cur / out / res2 / w / bias are not used; block k of the launch publishes
// r.epoch + 8 k + 1 .. + 5, so the next launch's epoch is at least r.epoch + 8 nblocks.
struct RdbChainBlock {
    const void* cur;
    void* out;
    const void* res2;
    const void* w[5];
    const float* bias[5];
};
hipError_t launch_rdb_f16x2_chain(const RdbLaunch& r, const RdbChainBlock* table, int nblocks, hipStream_t s);

// bf16 dense block with the working set resident in LDS (rdb_bf16_strip.hip): a workgroup owns a 16-column strip of an
// image and sweeps it top to bottom in positions of 12 rows; x1..x4 never leave the CU except for the strips' edge columns.
constexpr int STRIP_BH = 12, STRIP_BW = 16;
constexpr int STRIP_XCH_BYTES = 2 * 2 * 4 * STRIP_BH * 128;   // edge-column mailboxes of one strip
// An edge-column granule carries the tag epoch + position * 8 + layer (layer 1..4; the position is one of the IMAGE's own grid,
// pos0 .. pos1 - 1 of an item, not a time of the schedule), and a launch owns the tags [epoch, epoch + STRIP_EPOCH_STEP): the
// last position of an image is at most STRIP_EPOCH_STEP / 8 - 1, so the largest end position of an item the tags can tell apart:
constexpr unsigned STRIP_EPOCH_STEP = 2048;
constexpr int STRIP_MAX_POS1 = (int)(STRIP_EPOCH_STEP / 8);
static_assert((unsigned)(STRIP_MAX_POS1 - 1) * 8u + 4u < STRIP_EPOCH_STEP, "a tag of the last position runs into the next launch's");
struct StripSchedule {
    std::vector<int> items;      // 8 ints per item: image | mailbox group << 16, strip, image height, image width, first position, end
                                 // position, first output row stored, end row (a row segment of the strip; whole images: 0, npos, 0, h)
    std::vector<int> wg_first;   // [grid + 1]
    int grid = 0, smax = 0, makespan = -1;
    int nvimg = 0;               // mailbox groups (image segments): the exchange buffer holds nvimg * smax * STRIP_XCH_BYTES
    double efficiency = 0.0;     // strip positions of work / (compute units x makespan)
};
// n images of hw[2i] x hw[2i+1] internal pixels -> the packing (makespan < 0: the kernel does not apply).  seg_len: positions per row
// segment at most (0: chosen by the packer, < 0: images are never cut)
StripSchedule strip_schedule(int n, const int* hw, int cus, int seg_len = 0);
// Does the kernel run this packing?  It depends on the images alone, never on their company: a packing exists (no image wider
// than the workgroups), every item's end position fits the tag space (STRIP_MAX_POS1) and the item words hold their fields
// (image < 65536, mailbox group < 32768).  The one answer of the forward (strip_plan_for) and of nesr_strip_schedule.
int strip_largest_pos1(const StripSchedule& S);
bool strip_plan_applies(const StripSchedule& S);
// The lists walked on the host: a unit (the strips of one image segment) starts when all of its workgroups have reached it.
// -> the largest number of positions a workgroup idles in front of its next item, the walk's makespan in *makespan; -1 if the
// walk stops with items left (a cycle of waits: no global order of the units that every list respects)
int strip_max_wait(const StripSchedule& S, int* makespan);
size_t strip_weight_bytes();
void pack_strip_weights(const float* const w[5], uint16_t* dst, bool f16);   // conv1..conv5 OIHW f32 of one dense block -> bf16 | f16
struct StripLaunch {
    const void* cur; long long chunk_bytes; void* out; const void* res2;
    float s1, s2;
    const void* wstream; const float* bias;       // device: pack_strip_weights image, [192] f32 (conv1..4: 32 each, conv5: 64)
    int H, W;                                     // slot geometry of the batch buffers
    const void* items; const int* wg_first;       // device copies of the schedule
    int grid, smax;
    void* xch;                                    // nvimg * smax * STRIP_XCH_BYTES
    unsigned epoch;                               // strictly increasing by >= STRIP_EPOCH_STEP per launch
    unsigned* abort_flag;
    unsigned long long timeout_ticks;
    int debug_drop;                               // test hook: this many workgroups of the launch never start
    int f16;                                      // 0: bf16 operands; 1: f16 operands (pack_strip_weights(..., true))
    unsigned* status;                             // f16: the range word (ConvArgs::status); separate from abort_flag
};
hipError_t launch_rdb_bf16_strip(const StripLaunch& r, hipStream_t s);

// Persistent trunk (conv3x3_mfma.hip): all dense-block convs of the 23 RRDBs in ONE cooperative
// launch.  Workgroups keep their tiles from layer to layer and synchronise with their 8
// neighbouring tiles only (per-tile progress counters, agent-scope release/acquire), instead of 345
// kernel boundaries at which the whole chip drains and refills.
struct TrunkLayer {
    int in_buf, out_buf, res1_buf, res2_buf;   // 0..2 = the rotating 192-channel buffers P,Q,R; -1 = none
    int cin, coutp, out_coff, lrelu;
    float s1, s2;
    const void* w;
    const float* bias;
};
struct TrunkArgs {
    const TrunkLayer* layers;   // device array
    int nlayers;
    void* buf[3];
    Map map;                    // addressing of P,Q,R (192 channels each)
    int n, h, w;
    unsigned* progress;         // [tiles] layers completed per tile, zeroed before the launch
    unsigned* abort_flag;       // set by a workgroup whose bounded wait timed out
    const void* zeros;
};
// returns the workgroup count it would launch (0 = the persistent form does not apply)
hipError_t launch_trunk_persist(const TrunkArgs& t, bool bf16, hipStream_t s);

// input packers (pack.hip): NCHW f32 (+ pixel_unshuffle) -> NHWC with `cp` channels (zero padded)
struct PackArgs {
    const void* src;     // f32 NCHW [n][c][hin][win]   or u8 HWC [hin][win][3] (n == 1)
    int src_u8;          // 1: u8 HWC source, value/255, optional channel flip
    int flip;
    int n, c, hin, win;
    int unshuffle;       // 1, 2 or 4
    void* dst;           // feature map with cp channels (zero padded), addressed through dst_map
    Map dst_map;
    int cp;
    int bf16;            // destination layout: 0 f32 NHWC (KG = 8), 1 bf16 blocked (KG = 16), 2 f16 hi|lo blocked (KG = 16),
                         // 3 f16 blocked (KG = 16)
    unsigned* status;    // as ConvArgs::status (layouts 2 and 3); may be null
};
hipError_t launch_pack_input(const PackArgs& a, hipStream_t s);
hipError_t launch_status_latch(unsigned* status, hipStream_t s);   // range word of an unchecked earlier forward: word 0 -> word 3

// the NESR pipeline's network input (nesr12.hip): a window of an RGB u8 HWC frame -> conv_first's 12 channels (+ 4 of zero padding)
struct Pack12Args {
    const uint8_t* src;      // the frame: [rows][pixels][3] RGB u8, rows src_stride bytes apart
    long long src_stride;
    int y0, x0, h, w;        // the window (h, w >= 2): the blur's border is the window's edge
    int mode;                // NESR_INPUT_12CH | NESR_INPUT_3CH_X4
    void* dst;               // as PackArgs: feature map with cp = 16 channels, addressed through dst_map
    Map dst_map;
    int cp;
    int bf16;                // destination layout, as PackArgs::bf16
    unsigned* status;        // as PackArgs::status
};
hipError_t launch_pack_nesr12(const Pack12Args& a, hipStream_t s);

// Row bands inside one process (band_exchange.hip): the first / last edge rows of a band's feature map, gathered from the context's
// activation layout into the packed form of nesr_band_rows and written straight into the neighbour contexts' landing buffers (plain
// pointers on the same device, peer-mapped ones on another).  A side is `nseg` segments `seg_stride` bytes apart, each of `npieces`
// pieces of `piece_vecs` 16-byte vectors `piece_stride` bytes apart; the destination is contiguous.  src[i] == null: nothing for side i.
struct EdgePush {
    const char* src[2];      // [0] the first band rows (they go to the band above), [1] the last band rows
    char* dst[2];
    long long seg_stride, piece_stride;
    int nseg, npieces, piece_vecs;
};
hipError_t launch_band_push_edges(const EdgePush& a, hipStream_t s);

// all tiles of a frame at once (pack.hip): u8 HWC frame -> float NCHW tile slots (cut), float NCHW tile outputs -> u8 (paste)
constexpr int TILE_IO_MAX = 64;
struct TileIo {
    uint8_t* frame;       // cut: the frame (read); paste: base of the destination
    int frame_w;          // cut: pixels per frame row
    float* tiles;         // [n][3][Hs][Ws]
    int Hs, Ws;
    int flip, round;
    int desc[8 * TILE_IO_MAX];   // per tile: cut {y0, x0, h, w}; paste {crop y, crop x, h, w, row pitch (bytes), offset lo, offset hi}
};
hipError_t launch_cut_tiles(const TileIo& t, int n, int maxh, int maxw, hipStream_t s);
hipError_t launch_paste_tiles(const TileIo& t, int n, int maxh, int maxw, hipStream_t s);

// cv2.fastNlMeansDenoising (template 7, search 21) on [C][H][W] u8 planes taken as one C-channel image (imgproc.hip)
hipError_t launch_nl_means(const uint8_t* src, int C, int H, int W, const int* lut, int nbins, int shift, uint8_t* dst, hipStream_t s);

// cv2 CLAHE on one u8 plane (imgproc.hip): th x tw = tile size of the (virtually) padded image, clip = max(int(clipLimit * th * tw / 256), 1),
// scale = 255 / (th * tw), inv_th / inv_tw = 1 / th, 1 / tw as floats; lut: gx * gy * 256 floats of device scratch
hipError_t launch_clahe(const uint8_t* src, int h, int w, int gx, int gy, int th, int tw, int clip, float scale, float inv_th, float inv_tw, float* lut,
                        uint8_t* dst, hipStream_t s);

// Lab conversions (filters.hip): channel c of pixel i at src[c][i * src_step] (HWC: base + c, step 3; planar: plane c, step 1); mode0 then,
// unless negative, mode1 on the u8 result (NESR_LAB_* bits without NESR_LAB_PLANAR)
struct LabArgs {
    const uint8_t* src[3];
    uint8_t* dst[3];
    size_t n;
    int src_step, dst_step;
    int mode0, mode1;
};
hipError_t launch_lab(const LabArgs& a, hipStream_t s);

// cv2.GaussianBlur's 8-bit fixed-point path on HWC u8 (filters.hip): k[0 .. 2r] integer taps summing to 256, C = 1 or 3, dst != src
constexpr int GAUSS_MAX_RADIUS = 15;
struct GaussTaps {
    int r;
    int k[2 * GAUSS_MAX_RADIUS + 1];
};
hipError_t launch_gaussian(const uint8_t* src, int H, int W, int C, const GaussTaps& taps, uint8_t* dst, hipStream_t s);

// the adaptive unsharp mask of _postprocess_image on HWC RGB u8 (filters.hip): taps of the sigma 2 and sigma 3 blurs, dst != src
struct SharpenTaps {
    int k2[13];
    int k3[19];
};
hipError_t launch_postprocess(const uint8_t* src, int H, int W, const SharpenTaps& taps, uint8_t* dst, hipStream_t s);
// the same kernel selecting by the 3 x 3 dilate of mask [H][W] u8 {0, 1} (the image half of _segment_and_enhance); k2 is not read
hipError_t launch_segment_sharpen(const uint8_t* src, int H, int W, const SharpenTaps& taps, const uint8_t* mask, uint8_t* dst, hipStream_t s);

// _ensemble_results on n <= ENSEMBLE_MAX u8 images of `total` bytes each (filters.hip): the float32 mean with weight w, truncated
constexpr int ENSEMBLE_MAX = 8;
struct EnsembleArgs {
    const uint8_t* img[ENSEMBLE_MAX];
    uint8_t* out;
    size_t total;
    int n;
    float w;
};
hipError_t launch_ensemble(const EnsembleArgs& a, hipStream_t s);

// cv2.resize (resize.hip).  src / dst: base pointer + row stride in bytes, pixels of a row contiguous, C interleaved channels.
// Lanczos-4 (u8: C = 1, 3, 4, fixed point; u16: float32): xtab / ytab = device tables of dst_w / dst_h positions, int32 first tap
// (i0 - 3, unclamped) for every position, then 8 coefficients per position (u8: the 11-bit ints, u16: float32); a workgroup owns
// tx x ty outputs (tx a power of two <= 256) and lds_bytes of LDS: [stage | output tile] of region0 bytes, then the horizontal sums;
// stage_pitch / out_pitch = LDS bytes per staged source row / per output row (multiples of 4 that leave 3 bytes for the row's
// alignment); max_rows = source rows a tile reads at most.  Linear f32 (C = 1..4): tables = i0[n], i1[n], f[n] (float bits).
constexpr int RESIZE_LDS_BUDGET = 64 * 1024;      // per workgroup: two fit the 160 KiB of a CU
struct ResizeArgs {
    const unsigned char* src;
    unsigned char* dst;
    long long src_stride, dst_stride;
    int src_h, src_w, dst_h, dst_w, C;
    const int* xtab;
    const int* ytab;
    int tx, ty, max_rows, stage_pitch, out_pitch, region0, lds_bytes;
};
hipError_t launch_resize_lanczos4(const ResizeArgs& a, int elem_bytes, hipStream_t s);
// the other 8-bit interpolations of nesr_resize_cv_u8 (C = 1, 3, 4).  Cubic: the Lanczos kernel with 4 taps (tables: first tap i0 - 1,
// unclamped, then 4 11-bit coefficients per position; the tile plan counts 4 taps).  Nearest: tables = the source index per position.
// Linear: tables = the clamped first index per position, then 2 11-bit coefficients per position; both axes shrinking by exactly 2
// take cv2's area filter instead (no tables read).  Nearest and linear need no tile plan.
hipError_t launch_resize_cubic_u8(const ResizeArgs& a, hipStream_t s);
hipError_t launch_resize_nearest_u8(const ResizeArgs& a, hipStream_t s);
hipError_t launch_resize_linear_u8(const ResizeArgs& a, hipStream_t s);
hipError_t launch_resize_linear_f32(const ResizeArgs& a, hipStream_t s);

// Whole frames of every kind RealESRGANer.enhance takes (frame_io.hip): u8 / u16, gray / BGR / BGRA.  alpha_form: FRAME_ALPHA_RGB =
// three equal planes [3][H][W] (the network route, not flipped), FRAME_ALPHA_PLANE = one plane [H][W] (the linear-resize route;
// never rounded through fp16: it does not pass the network).
constexpr int FRAME_ALPHA_RGB = 0, FRAME_ALPHA_PLANE = 1;
struct FramePack {
    const unsigned char* src;   // [H][W] (C = 1) or [H][W][C] (C = 3, 4) samples of `bytes` bytes, rows src_pitch bytes apart
    long long src_pitch;
    int H, W, C, bytes;
    float max_range;            // 255 or 65535: v = (float)sample / max_range, correctly rounded
    int through_fp16;
    float* image;               // [3][H][W]: gray replicated, colour flipped BGR -> RGB
    float* alpha;               // C = 4: destination of the alpha samples in `alpha_form`, or null (not written)
    int alpha_form;
};
struct FrameUnpack {
    const float* image;         // [3] planes image_plane floats apart, rows image_row floats apart (a cropped view is read in place)
    long long image_plane, image_row;
    const float* alpha;         // C = 4: FRAME_ALPHA_RGB: three planes like `image`; FRAME_ALPHA_PLANE: one plane, rows alpha_row apart
    long long alpha_plane, alpha_row;
    int alpha_form;
    int H, W, C, bytes;         // the finished frame: [H][W] (C = 1) or [H][W][C] samples of `bytes` bytes, rows dst_pitch bytes apart
    float max_range;
    int through_fp16;           // the network outputs pass through fp16 once before the clamp
    unsigned char* dst;
    long long dst_pitch;
};
hipError_t launch_pack_frame(const FramePack& p, hipStream_t s);
hipError_t launch_unpack_frame(const FrameUnpack& u, hipStream_t s);

// feature map (channels [0,c)) -> planar f32 NCHW; used by the single-layer test hook
hipError_t launch_nhwc_to_nchw(const void* src, int kind /* as PackArgs::bf16 */, Map map, int n, int c, int h, int w, float* dst, hipStream_t s);

}  // namespace nesr

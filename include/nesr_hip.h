/*
 * nesr_hip.h -- C ABI of libnesr_hip.so: the MI355X (gfx950) Real-ESRGAN / RRDBNet inference path.
 *
 * The reference (gddickinson/neural_enhanced_super_resolution) is pure Python and has no FFI of
 * its own; the arithmetic of this path lives in the un-vendored pip packages basicsr (RRDBNet)
 * and realesrgan (RealESRGANer).  Each entry point below names the reference interface it
 * stands behind (paths relative to the reference root).  The Python host side
 * (neural_enhanced_super_resolution_amd/) binds these with ctypes and presents the
 * RRDBNet / RealESRGANer objects the reference constructs at nesr/nesr.py:216-229 and
 * standalone/direct_esrgan.py:104-127.
 *
 * Conventions: every function returns 0 on success and a negative code on failure; the message
 * is available from nesr_last_error() (thread-local).  No exception crosses the ABI.  Device
 * pointers are caller-owned (e.g. torch tensors' data_ptr()); the context owns packed weights
 * and its workspace.  `stream` is a hipStream_t passed as void* (NULL = default stream); all
 * device work is enqueued on it asynchronously.  One in-flight call per context
 * (the reference calls from one thread at a time: main thread or one QThread,
 * nesr/gui/app.py:72,1732-1749); hipSetDevice is done on entry so any thread may call.
 */
#ifndef NESR_HIP_H
#define NESR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nesr_ctx nesr_ctx;

/* NESR_DTYPE_F32_WINOGRAD: f32 storage and f32 matrix-core arithmetic, the feature-map 3x3 convs
 * evaluated by Winograd F(2x2,3x3) (2.25x less matrix work; a few ulps per layer away from the
 * direct form, far inside the 1e-3 output tolerance). */
/* NESR_DTYPE_F32_SPLIT: f32 in, f32 out, f32 accumulation; every conv operand is carried as a pair of halves,
 * x = hi + lo * 2^-11 (hi = f16(x), lo = f16((x - hi) * 2^11)), and each product is three f16 MFMAs
 * (hi*hi + hi*lo + lo*hi), see conv3x3_f16x2.hip.  The pair holds 22 significant bits for 6.1e-5 <= |x| <= 65504
 * and an absolute 2^-35 below; a value outside +-65504 or a non-finite one does NOT fit: nesr_finalize_weights
 * rejects such a weight (NESR_ERR_RANGE), and such an input or activation raises the context's range flag --
 * the float output of THAT forward is then NaN and nesr_check_range / nesr_check_status return NESR_ERR_RANGE.  The flag is
 * scoped to one forward: a caller of nesr_forward that never asks does not get NaN for later, valid frames; the unreported
 * condition is latched and returned (once) by the next nesr_check_range.  Callers of nesr_forward MUST call nesr_check_range
 * (or nesr_check_status) before trusting an output.
 * Whole-network max abs error vs an f64 evaluation 3e-6 on the bench weights (plain f32: 1e-6). */
/* NESR_DTYPE_F16: f16 storage and f16 MFMA operands (v_mfma_f32_{32x32x16,16x16x32}_f16), f32 accumulation and epilogue --
 * upstream's half=True numerics; the same kernels, layouts and batching as NESR_DTYPE_BF16 (three more significand bits).
 * Range contract, as for NESR_DTYPE_F32_SPLIT: f16 carries |x| <= 65504 only.  nesr_finalize_weights (and nesr_conv3x3)
 * reject a weight beyond that (NESR_ERR_RANGE); an input or stored activation that is non-finite or beyond +-65504 raises the
 * context's range word, the float output of THAT forward is NaN (an 8-bit output is invalid) and nesr_check_range /
 * nesr_check_status return NESR_ERR_RANGE, scoped and latched per forward as above -- never a silently saturated image.
 * The opt-in persistent trunk (NESR_TRUNK=persist) is f32 / bf16 only: an f16 context runs per-layer launches there;
 * nesr_forward_sharded_u8 takes bf16 contexts only. */
enum { NESR_DTYPE_F32 = 0, NESR_DTYPE_BF16 = 1, NESR_DTYPE_F32_WINOGRAD = 2, NESR_DTYPE_F32_SPLIT = 3, NESR_DTYPE_F16 = 4 };
enum { NESR_ROUND_TRUNC = 0, NESR_ROUND_NEAREST = 1 };

enum {
    NESR_OK = 0,
    NESR_ERR_ARG = -1,      /* bad argument / unsupported shape */
    NESR_ERR_HIP = -2,      /* a HIP runtime call failed */
    NESR_ERR_STATE = -3,    /* weights missing / not finalized */
    NESR_ERR_NOMEM = -4,
    NESR_ERR_RANGE = -5,    /* f16-pair fp32 form or f16 form: a weight, input or activation was non-finite or beyond +-65504 */
    NESR_ERR_NOFIT = -6,    /* nesr_jpeg_encode_u8: the file did not fit out_cap (what a caller reports after reading the status word) */
    NESR_ERR_UNSUPPORTED = -7, /* nesr_jpeg_parse: a valid JPEG file outside the supported list */
    NESR_ERR_BADFILE = -8   /* nesr_jpeg_parse: malformed segments; nesr_jpeg_decode_u8: a scan the device rejected (the status word) */
};

/*
 * Replaces: RRDBNet.__init__ (basicsr archs/rrdbnet_arch.py) as called at nesr/nesr.py:216,
 * standalone/direct_esrgan.py:104, standalone/superres_project.py:69.
 *   conv_first_in_ch : input channels of conv_first (3 for x4plus; 12 for x2plus and for the
 *                      nesr 12-channel quirk)
 *   unshuffle        : 0 = none (upstream scale=4), 2 = pixel_unshuffle(2) folded into the input
 *                      load (upstream scale=2), 4 = pixel_unshuffle(4) (upstream scale=1).
 *                      forward() then expects C = conv_first_in_ch / unshuffle^2 input channels.
 *   dtype            : one of NESR_DTYPE_* -- storage and arithmetic of activations/weights (accumulation is always f32).
 */
int nesr_create(nesr_ctx** out, int device_id, int conv_first_in_ch, int unshuffle, int num_feat,
                int num_block, int num_grow_ch, int num_out_ch, int dtype);

/* Activations of SRVGGNetCompact (upstream act_type 'prelu' | 'relu' | 'leakyrelu'; LeakyReLU's slope is 0.1). */
enum { NESR_ACT_PRELU = 0, NESR_ACT_RELU = 1, NESR_ACT_LEAKYRELU = 2 };

/*
 * Replaces: SRVGGNetCompact.__init__ (realesrgan archs/srvgg_arch.py), the network of the realesr-general-x4v3 (and its -wdn
 * twin), realesr-animevideov3 checkpoints the reference fetches (standalone/download-x3-model.py:77-116):
 *     body = conv3x3(in, F), act, (conv3x3(F, F), act) x num_conv, conv3x3(F, out * s * s)
 *     out  = pixel_shuffle(body(x), s) + nearest_upsample(x, s)
 * State dict: body.{2i}.weight / .bias for the convs, body.{2i+1}.weight [F] for each PReLU (none for relu / leakyrelu).
 *   num_feat 64, num_in_ch == num_out_ch == 3, upscale 2 or 4, 1 <= num_conv <= 1024, act_type one of NESR_ACT_*,
 *   dtype NESR_DTYPE_F32_SPLIT (f32 as f16 pairs, range word as for nesr_create), NESR_DTYPE_BF16 or NESR_DTYPE_F16 (bf16's kernels
 *   on f16 elements: upstream's half=True numerics; weights rounded to nearest even and refused beyond +-65504 at
 *   nesr_finalize_weights, the range word as for NESR_DTYPE_F32_SPLIT); anything else NESR_ERR_ARG.
 * On such a context nesr_load_weight, nesr_finalize_weights, nesr_num_tensors, nesr_forward (output [N, 3, sH, sW]),
 * nesr_forward_u8, nesr_workspace_bytes, nesr_reserve, nesr_forward_flops, nesr_set_kernel_timing / nesr_kernel_time_ms
 * (the num_conv body convs), nesr_check_status, nesr_check_range and nesr_destroy work as documented for nesr_create;
 * nesr_set_size_independent and nesr_set_concurrent are accepted (the kernel choice never depends on size or batch);
 * the RRDB-only entries (ragged, band, sharded, fused / strip switches, preferred batch) return NESR_ERR_ARG.
 */
int nesr_create_compact(nesr_ctx** out, int device_id, int num_in_ch, int num_out_ch, int num_feat, int num_conv, int upscale,
                        int act_type, int dtype);

/*
 * Replaces: model.load_state_dict(loadnet[keyname], strict=True) in RealESRGANer.__init__
 * (realesrgan utils.py), reached from nesr/nesr.py:220-229, standalone/direct_esrgan.py:118-127.
 * `key` is the upstream state_dict name ("conv_first.weight", "body.0.rdb1.conv1.bias", ...),
 * `data` a HOST pointer to f32 (weights OIHW, bias [O]); it is repacked and copied, the caller
 * keeps ownership.  Unknown key or shape mismatch -> NESR_ERR_ARG (strict=True semantics).
 */
int nesr_load_weight(nesr_ctx* ctx, const char* key, const float* data, const int64_t* shape, int ndim);

/* strict=True: fails with NESR_ERR_STATE (message lists the first missing keys) unless every
 * tensor of the architecture was loaded. Uploads packed weights to the device. */
int nesr_finalize_weights(nesr_ctx* ctx);

/* Number of state_dict tensors the architecture expects (702 for num_block=23). */
int nesr_num_tensors(const nesr_ctx* ctx);

/*
 * Replaces: RRDBNet.forward -- `self.model(self.img)` in RealESRGANer.process/tile_process and
 * `model(img_12ch)` at nesr/nesr.py:891,935.
 *   x_dev : NCHW f32 [N, C, H, W] contiguous device memory
 *   y_dev : NCHW f32 [N, num_out_ch, 4*H/u, 4*W/u] (u = unshuffle or 1) device memory
 * H and W must be multiples of the unshuffle factor (upstream asserts the same).
 */
int nesr_forward(nesr_ctx* ctx, const void* x_dev, int N, int C, int H, int W, void* y_dev, void* stream);

/*
 * Fused image path: replaces `img/255`, cv2 BGR<->RGB flips, HWC->CHW,
 * RRDBNet.forward, clamp(0,1), x255 and the quantiser of RealESRGANer.enhance
 * (round_mode NESR_ROUND_NEAREST, flip_rgb 1) or of nesr/nesr.py:851-857,894-901
 * (NESR_ROUND_TRUNC, flip_rgb 0).
 *   in_hwc_dev  : u8 [H, W, 3] device memory;  out_hwc_dev : u8 [4H/u, 4W/u, 3] device memory.
 * Requires conv_first_in_ch / unshuffle^2 == 3 and num_out_ch == 3.
 */
int nesr_forward_u8(nesr_ctx* ctx, const uint8_t* in_hwc_dev, int H, int W, uint8_t* out_hwc_dev,
                    int flip_rgb, int round_mode, void* stream);

/*
 * Forward pass on N images of DIFFERENT sizes in one batch: the tiles of one frame as realesrgan's tile_process cuts them
 * (`for y in range(tiles_y): for x in range(tiles_x): ... self.model(input_tile)`, called from
 * standalone/direct_esrgan.py:148 with tile=512, tile_pad=10 -- interior tiles 532 x 532, edge and corner tiles smaller).
 * Image i lies in the top-left hw[2i] x hw[2i+1] pixels of slot i of x_dev ([N, C, H, W] f32; the rest of a slot is
 * ignored) and its output in the top-left of slot i of y_dev ([N, num_out_ch, 4H/u, 4W/u]; the rest is not written).
 * Each image is evaluated as an image of its own -- its borders are the zero padding of every conv -- with the values
 * nesr_forward gives it alone (see nesr_set_size_independent).  hw: host array of N (height, width) pairs, multiples of
 * the unshuffle factor, 1 <= N <= 64.  compute dtype bf16 or f16 only (NESR_ERR_ARG otherwise: the f32 forms batch equal shapes).
 */
int nesr_forward_ragged(nesr_ctx* ctx, const void* x_dev, int N, int C, int H, int W, const int* hw, void* y_dev, void* stream);

/* Choose kernels by arithmetic only, never by image size or batch composition, so that an image's values are the same bits
 * alone, in an equal-shape batch and in a ragged batch -- and on any rank of a sharded frame, whatever its share.  bf16: the dense
 * blocks always run as the LDS-resident kernel (rdb_bf16_strip_kernel; a batch too small to fill the device is cut into row
 * segments, which does not change a bit), the other layers as the large-tile kernel also for small images.  RealESRGANer sets it
 * for a tiling wrapper.  Off by default: a plain context picks whichever form is faster for the batch at hand (the two bf16
 * forms agree to bf16 resolution, not bit for bit). */
int nesr_set_size_independent(nesr_ctx* ctx, int on);

/* Device bytes of activation workspace forward() needs for a batch of N frames of H x W input. */
size_t nesr_workspace_bytes(const nesr_ctx* ctx, int N, int H, int W);

/* Pre-allocates the workspace (forward() grows it on demand otherwise, which synchronises). */
int nesr_reserve(nesr_ctx* ctx, int N, int H, int W);

/* Batch size <= max_batch (frames of H x W input evaluated by one forward()) whose trunk launches
 * fill the device's compute units most evenly -- used by RealESRGANer.tile_process to group the
 * equal-shaped tiles of upstream's tile grid. */
int nesr_preferred_batch(const nesr_ctx* ctx, int H, int W, int max_batch);

/* Algorithmic FLOPs (2 x MACs) of one forward() on N frames of H x W input. */
double nesr_forward_flops(const nesr_ctx* ctx, int N, int H, int W);

/*
 * Banded evaluation: the exact (seamless) multi-GPU mode of SURVEY.md section 8(e).  Stands behind the same
 * reference call as nesr_forward -- `self.model(img)` on a whole frame, nesr/nesr.py:887-891 with tile=0
 * (nesr/nesr.py:224) -- when the frame is split into row bands, one per rank.  A rank holds its band plus `apron`
 * rows of its neighbours (N = 1, input [1,C,H,W] NCHW f32 including the apron rows) and runs the stages in order:
 *     nesr_band_begin                       pixel_unshuffle + conv_first
 *     nesr_band_rdb(i), i = 0 .. 3*num_block-1   the five convs of RDB i (RRDB i/3, dense block i%3)
 *     nesr_band_tail                        conv_body .. conv_last  ->  [1,num_out_ch,4h,4w] f32
 * Every 3x3 conv spoils one more row at a band edge that is not a frame edge, so before a stage the caller
 * overwrites the apron rows of the feature map the stage reads with the neighbours' band rows: buffer i%3 before
 * nesr_band_rdb(i) (5 rows), buffers 0 and 3 before nesr_band_tail (3 rows).  nesr_band_rows moves rows
 * [row0, row0+nrows) of the num_feat-channel slice of a buffer (0,1,2 = the rotating dense-block buffers, 3 = the
 * conv_first output kept for the trunk skip) to/from a contiguous staging buffer of nrows * nesr_band_row_bytes
 * bytes, in the context's own element layout (opaque: only ever handed to another rank's nesr_band_rows).
 * neural_enhanced_super_resolution_amd/banded.py is the reference-side protocol (RCCL point-to-point).
 */
/*
 * The same stages with the exchange taken off the critical path (banded.py's default protocol):
 *   nesr_band_rdb_phase(i, 0, ...)   conv1..conv4 of RDB i, and conv5 on the `edge_rows` band rows next to each apron --
 *                                     the rows the neighbours wait for (top / bottom = apron rows of this band image)
 *   nesr_band_pack_edges             those rows of the buffer RDB i wrote -> two caller-owned staging buffers (one call;
 *                                     the caller sends them, e.g. RCCL point-to-point on a side stream)
 *   nesr_band_rdb_phase(i, 1, ...)   conv5 on the band rows in between, while the edge rows travel
 *   nesr_band_unpack_aprons          the neighbours' rows -> this band image's apron rows, before RDB i + 1
 * Values are those of nesr_band_rdb (row ranges of the same kernel).  Row-range launches exist for NESR_DTYPE_F32_SPLIT;
 * for the other dtypes phase 0 runs the whole block and phase 1 nothing (same protocol, no overlap).
 */
int nesr_band_rdb_phase(nesr_ctx* ctx, int index, int phase, int top, int bottom, int edge_rows, void* hip_stream);
int nesr_band_pack_edges(nesr_ctx* ctx, int buffer, int top, int bottom, int nrows, void* top_dst, void* bottom_dst, void* hip_stream);
int nesr_band_unpack_aprons(nesr_ctx* ctx, int buffer, int top, int bottom, int nrows, const void* top_src, const void* bottom_src,
                            void* hip_stream);
int nesr_band_begin(nesr_ctx* ctx, const void* x_dev, int C, int H, int W, void* hip_stream);
int nesr_band_rdb(nesr_ctx* ctx, int index, void* hip_stream);
int nesr_band_tail(nesr_ctx* ctx, void* y_dev, void* hip_stream);
size_t nesr_band_row_bytes(const nesr_ctx* ctx);
int nesr_band_rows(nesr_ctx* ctx, int buffer, int row0, int nrows, void* staging_dev, int write, void* hip_stream);

/*
 * Row bands inside ONE process: an untiled frame on RealESRGANer(devices=[...]) (csrc/band_exchange.hip, csrc/band_api.cpp; DESIGN.md
 * section 6).  The contexts of the bands know each other, a band's edge rows are written straight into its neighbours' memory, and the
 * whole frame runs below Python.  Every entry stands behind `self.model(img)` on a whole frame (nesr/nesr.py:224, 887-891).
 *
 * nesr_band_link (nesr/nesr.py:224, 887-891): makes `up` the band above `ctx` and `down` the band below (either may be null: a frame
 *   edge); both directions of a link are set, earlier links of the three contexts on those sides are dropped.  A link is WRITTEN
 *   DIRECTLY by the push kernel when both contexts are on one device (the plain pointer) or the runtime grants peer access
 *   (hipDeviceEnablePeerAccess, asked once here); otherwise it is STAGED: the existing pack, then hipMemcpyPeerAsync -- the same bytes.
 *   Landing buffers are allocated when the first rows of a width are pushed.  NESR_ERR_ARG: an SRVGGNetCompact context, a neighbour of
 *   another geometry or dtype, ctx as its own neighbour, one context on both sides.  nesr_band_unlink drops both links of ctx
 *   (nesr_destroy does so too).  nesr_band_link_state: bit 0 / 1 = an upper / lower neighbour exists, bit 2 / 3 = that link is written
 *   directly, bit 4 / 5 = the neighbour is on another device; negative: an error code.  nesr_band_set_staged(ctx, 1) makes every link
 *   of ctx staged whatever the devices allow (A/B runs and tests of that route; 0: decide again).
 * nesr_band_push_edges (nesr/nesr.py:224, 887-891): one launch of band_push_edges on `hip_stream`.  The first `edge_rows` band rows of
 *   `buffer` (rows [top, top + edge_rows) of the band image; the rows nesr_band_pack_edges selects) go to the upper neighbour's landing
 *   buffer of `parity` (0 | 1), the last ones to the lower neighbour's; 1 <= edge_rows <= 6.  Both neighbours must hold a band image of
 *   the same width (nesr_band_begin).  The kernel waits for nothing: the CALLER orders it after the neighbour's nesr_band_land_aprons of
 *   the same parity two steps earlier, and the neighbour's nesr_band_land_aprons after it (hipEventRecord / hipStreamWaitEvent).
 * nesr_band_land_aprons (nesr/nesr.py:224, 887-891): the receiver's side: landing buffers of `parity` -> the `edge_rows` apron rows next
 *   to the band on each linked side, of `buffer` and of every buffer whose bit is set in also_mask (8: conv_first's copy, after step 0).
 * nesr_band_plan (nesr/nesr.py:224, 887-891; host only): the bands of `internal_rows` trunk rows over n contexts, lo_hi[2r], lo_hi[2r+1]
 *   = [lo, hi) of band r -- banded.band_split: even boundaries, NESR_ERR_ARG when a band would be shorter than the 6-row apron
 *   (cap: (lo, hi) pairs lo_hi holds, >= n).
 * nesr_forward_banded_u8 (nesr/nesr.py:224, 887-891): nesr_forward_u8 of one frame as n row bands, band r on ctxs[r].  frame_u8 and out_u8
 *   are on ctxs[0]'s device; a band's input rows (with aprons) are read in place there or copied to its device, then nesr_band_begin's
 *   stage, 1 + 3 num_block exchange steps (phase 0, push, phase 1, land) and nesr_band_tail's stage with conv_last's own quantiser; the
 *   band's rows without aprons are copied into out_u8.  streams: n hipStream_t, band r's work goes to streams[r]; null: streams the
 *   contexts own.  On return everything is enqueued and the frame is complete behind streams[0] (band 0's stream); nothing is
 *   allocated or synchronised after the first frame of a geometry.  The f32 forms only (NESR_DTYPE_F32, _F32_WINOGRAD, _F32_SPLIT):
 *   out_u8 is byte for byte nesr_forward_u8's.  Bands never run the persistent dense-block kernel.  Call nesr_check_range on EVERY
 *   context before trusting out_u8: the range word is per context, and a band that overflowed spoils its own rows only.
 * nesr_forward_banded (nesr/nesr.py:224, 887-891): the float twin, nesr_forward for N = 1: x_dev [1, C, H, W], y_dev [1, num_out_ch,
 *   4H/u, 4W/u] f32 on ctxs[0]'s device.
 */
int nesr_band_link(nesr_ctx* ctx, nesr_ctx* up, nesr_ctx* down);
int nesr_band_unlink(nesr_ctx* ctx);
int nesr_band_link_state(const nesr_ctx* ctx);
int nesr_band_set_staged(nesr_ctx* ctx, int on);
int nesr_band_push_edges(nesr_ctx* ctx, int buffer, int top, int bottom, int edge_rows, int parity, void* hip_stream);
int nesr_band_land_aprons(nesr_ctx* ctx, int buffer, int also_mask, int top, int bottom, int edge_rows, int parity, void* hip_stream);
int nesr_band_plan(int internal_rows, int n, int* lo_hi, int cap);
int nesr_forward_banded_u8(nesr_ctx** ctxs, int n, const uint8_t* frame_u8, int H, int W, int flip_rgb, int round_mode, uint8_t* out_u8, void** streams);
int nesr_forward_banded(nesr_ctx** ctxs, int n, const void* x_dev, int C, int H, int W, void* y_dev, void** streams);

/* Hint: forwards of this context run while other contexts of the process use the same device (several frames or
 * tile groups in flight on different streams).  Changes kernel selection only, never a value. */
int nesr_set_concurrent(nesr_ctx* ctx, int concurrent);

/*
 * The dense blocks of small f32 frames (rdb_f16x2_kernel) and of bf16 tile batches (rdb_bf16_strip_kernel) run as PERSISTENT
 * launches whose workgroups wait for one another; they need every workgroup resident, i.e. the device to themselves.  Inside a
 * process such launches of different contexts / streams are serialised per device (an event wait, no host blocking).  Against
 * another process nothing can order them: every wait is bounded by wall clock (200 ms; NESR_FUSED_TIMEOUT_MS), a workgroup
 * that gives up raises an abort word that ends all other waits of that forward at once, nesr_check_range / nesr_check_status
 * then return NESR_ERR_HIP for it, and the context switches to per-layer launches for good (f32: the same values bit for bit;
 * bf16: the per-layer kernels' values) -- re-run the frame.  nesr_set_fused(ctx, 0 | 1) makes that choice by hand;
 * nesr_fused_state returns bit 0 = persistent launches enabled, bits 1.. = forwards that gave up so far; a NEGATIVE value is an
 * error code, not a bitmask (NESR_ERR_ARG on an SRVGGNetCompact context, which has no persistent launches).
 * nesr_debug_fault is a TEST HOOK: the next persistent launch leaves out its last `drop_workgroups` workgroups (their
 * neighbours' waits must end in the abort word within the time limit).
 * Stands behind the same reference calls as nesr_forward (nesr/nesr.py:887-891, standalone/direct_esrgan.py:148).
 */
int nesr_set_fused(nesr_ctx* ctx, int on);
int nesr_fused_state(const nesr_ctx* ctx);
int nesr_debug_fault(nesr_ctx* ctx, int drop_workgroups);

/*
 * rdb_bf16_strip_kernel: which workgroup runs which 16-column strips of which image, in which order, is a host-side packing.
 * Read when a context is created: NESR_STRIP = -1 | 0 | 1 (auto: size-independent contexts and batches that fill the device;
 * never; wherever the kernel applies), NESR_STRIP_SEG = n (positions of 12 rows per row segment of a strip at most; 0: the packer
 * decides, the default; -1: images are never cut), NESR_STRIP_CUS = k (the workgroup count the packer plans for, clamped to
 * 1 .. the device's compute units; default: all of them -- fewer workgroups put more items on each, the values do not change).
 * The kernel applies to a batch when no image is wider than 16 k columns and none has more than 256 positions
 * (ceil((h + 4) / 12) of its trunk height h: the edge-column tags of a launch hold position * 8 + layer below 2048).  That
 * depends on the images alone, so a size-independent context gives an image one arithmetic in every batch.
 * nesr_strip_schedule is host only (no device, no context): the packing of n images of hw[2i] x hw[2i+1] trunk pixels for `cus`
 * workgroups.  items receives 8 ints per item (image | mailbox group << 16, strip, image height, image width, first position,
 * end position, first row stored, end row), wg_first the grid + 1 list bounds; info[10] = makespan (positions; -1: no packing),
 * grid, smax (most strips of an image), mailbox groups, items, applies (0 | 1: what the forward decides), max_wait (most
 * positions a workgroup idles in front of its next item, by a walk of the lists; -1: the walk found a cycle), the walk's
 * makespan, the largest end position of an item, the largest one the tag space admits; *efficiency = strip positions of work /
 * (cus x makespan).  info and efficiency are written even where the buffers are too small (NESR_ERR_ARG): info[4] and info[1] + 1
 * are the capacities to come back with.
 */
int nesr_strip_schedule(int n, const int* hw, int cus, int seg_len, int* items, int items_cap, int* wg_first, int wg_cap, int* info,
                        double* efficiency);

/*
 * Where rdb_f16x2_kernel applies to every dense block of a whole-frame forward, the trunk goes out as ONE launch of
 * rdb_f16x2_chain_kernel: the same block body run 3 num_block times, the block boundary a nine-neighbour wait on the progress words
 * where it was a kernel boundary (the values are the same bit for bit).  The row-band and single-block entries (nesr_band_*) keep one
 * launch per block.  NESR_RDB_CHAIN=0 | 1 (default 1) sets the choice for new contexts, for A/B runs; any other value is refused.
 * nesr_rdb_chain_state: what the LAST whole-frame forward of the context sent through the fused f32 dense-block kernels: kernel
 * launches and dense blocks -- 1 and 3 num_block chained, 3 num_block and 3 num_block with one launch per block, 0 and 0 with
 * per-layer launches.  For the dense-block routes the launch counter of nesr_kernel_time_ms counts DENSE BLOCKS dispatched per
 * fused route (one per block of a chained launch, as for one launch per block), five per block for per-layer launches.
 * nesr_rdb_chain_table is host only (no device, no context): the chained launch's table for num_block RRDBs as the forward builds it,
 * from the addresses of the three trunk buffers and of every layer's packed weights and bias (1 + 15 num_block each, indexed like the
 * network's layers: conv_first, then body.b.rdbR.convK); table receives 3 num_block entries of 13 addresses: cur, out, res2 (0: none),
 * w[5], bias[5].
 */
int nesr_rdb_chain_state(const nesr_ctx* ctx, int* kernel_launches, int* blocks);
int nesr_rdb_chain_table(int num_block, const uint64_t* buffers, const uint64_t* layer_w, const uint64_t* layer_b, uint64_t* table);

/*
 * conv_up1 / conv_up2 convolve a nearest-x2 upsample.  Every output parity (py, px) of such a layer reads a 2x2 neighbourhood
 * of the low-resolution input only, so NESR_DTYPE_F32_SPLIT contexts run the layer as four 2x2-tap convolutions whose weights are
 * the 3x3 taps summed once in nesr_finalize_weights (f32, ky then kx ascending): 2.25x fewer multiply-adds.  The sums round
 * differently from the nine separate products, at the level of the pair format's own error (2^-22 relative per product).
 * nesr_set_upconv(ctx, NESR_UPCONV_3X3) selects the full 3x3 form on the upsampled image instead (the values of earlier
 * releases, for A/B runs); the environment variable NESR_UPCONV=3x3 | 2x2 sets the default of new contexts.  The choice
 * never depends on a shape.  The other compute forms always run the 3x3 form; nesr_upconv_state returns the mode in use
 * (negative: an error code; NESR_UPCONV_2X2 is returned only when the folded weights the launches need exist).  nesr_fold_upconv_weights is the host-side folding on its own (no device needed): OIHW f32
 * [cout][cin][3][3] -> folded[py][px][a][b][cout][cin], the weight of low-res pixel (y + py - 1 + a, x + px - 1 + b) for
 * output pixel (2y + py, 2x + px).
 */
#define NESR_UPCONV_3X3 0
#define NESR_UPCONV_2X2 1
int nesr_set_upconv(nesr_ctx* ctx, int mode);
int nesr_upconv_state(const nesr_ctx* ctx);
int nesr_fold_upconv_weights(const float* oihw, int cout, int cin, float* folded);

/*
 * conv_last has <= 4 real output channels.  NESR_DTYPE_F32_SPLIT contexts run it with one 16-channel MFMA column block per
 * workgroup instead of the 32-channel group's two (NESR_CONV_LAST_NARROW, the default): the same products accumulated in the
 * same order for the channels that are written, so the image is bit-identical, in both output modes; half the matrix work and
 * weight reads of the layer.  NESR_CONV_LAST_GENERAL selects the earlier geometry (A/B runs, and the reference of the bit-equality
 * tests); environment NESR_CONV_LAST=general | narrow sets the default of new contexts.  Other compute forms ignore it.
 * Both NESR_UPCONV and NESR_CONV_LAST accept exactly their two values; nesr_create fails with NESR_ERR_ARG on anything else.
 */
#define NESR_CONV_LAST_GENERAL 0
#define NESR_CONV_LAST_NARROW 1
int nesr_set_conv_last(nesr_ctx* ctx, int mode);

/*
 * Timing hook for bench.py's roofline leg: when enabled, forward() brackets the dominant kernel
 * family (the dense-block 3x3 convs) with hipEvents on the caller's stream; nesr_kernel_time_ms
 * returns the accumulated elapsed ms and launch count since the last call (synchronises those
 * events).  Off by default.
 */
int nesr_set_kernel_timing(nesr_ctx* ctx, int enable);
int nesr_kernel_time_ms(nesr_ctx* ctx, double* total_ms, int64_t* launches, double* flops);

/* Waits for the device and reports deferred failures of asynchronous work (the persistent trunk
 * kernel bounds every inter-workgroup wait and sets an abort word instead of hanging; the f16-pair
 * form's range flag, see nesr_check_range). */
int nesr_check_status(nesr_ctx* ctx);

/* Range / abort check of the forwards enqueued so far on `hip_stream` (NESR_DTYPE_F32_SPLIT, NESR_DTYPE_F16, and contexts whose dense blocks
 * ran as persistent launches; NESR_OK at once otherwise): waits for that stream only, returns NESR_ERR_RANGE if an input or activation did not fit the
 * (hi, lo) pair or the f16 value -- in the latest forward, or in an earlier one nobody asked about (the message says which; the latest output is
 * valid in the second case) -- and clears the flag.  Where the reference would hand back NaN/Inf pixels
 * (`model(img)` on diverged data, nesr/nesr.py:891) this path hands back NaN (float output) plus this error; the
 * Python wrappers call it after every device-to-host copy. */
int nesr_check_range(nesr_ctx* ctx, void* hip_stream);

void nesr_destroy(nesr_ctx* ctx);

/*
 * Tiled frames without the float canvas (SURVEY.md section 8(f) row 1 for frames larger than a tile).  Replaces, for all tiles of a
 * frame at once, RealESRGANer.enhance's `img.astype(float32) / 255`, BGR->RGB and tile_process's
 * `input_tile = self.img[:, :, y0:y1, x0:x1]` (nesr_cut_tiles_u8), and tile_process's paste of every tile's un-padded centre followed
 * by enhance's clamp(0, 1), RGB->BGR, x255, round (nesr_paste_tiles_u8); called from standalone/direct_esrgan.py:148 with
 * tile=512, tile_pad=10.
 *   through_fp16 : the values pass through fp16 once: upstream's RealESRGANer(half=True) hands the network an fp16 tensor
 *             (`self.img = self.img.half()`) and gets one back
 *   windows : host array, n x (y0, x0, h, w): tile i = frame[y0:y0+h, x0:x0+w] into the top-left of slot i of tiles_nchw_dev
 *             ([n, 3, Hs, Ws] f32; the rest of a slot is zeroed) -- the layout nesr_forward_ragged takes
 *   desc    : host array, n x (crop y, crop x, h, w, destination byte offset, destination row pitch in bytes): the h x w pixels
 *             at (crop y, crop x) of tile i's output (slot i of tiles_nchw_dev, [n, 3, Hs, Ws] f32) go to dst_dev + offset as u8 HWC
 *             rows `pitch` bytes apart -- a window of the frame's output canvas, or a packed per-tile buffer (multi-GPU gather)
 * 1 <= n <= 64.
 */
int nesr_cut_tiles_u8(int device_id, const uint8_t* frame_hwc_dev, int H, int W, int flip_rgb, int through_fp16, const int* windows, int n, int Hs,
                      int Ws, float* tiles_nchw_dev, void* hip_stream);
int nesr_paste_tiles_u8(int device_id, const float* tiles_nchw_dev, int n, int Hs, int Ws, const int64_t* desc, uint8_t* dst_dev, size_t dst_bytes,
                        int flip_rgb, int round_mode, int through_fp16, void* hip_stream);

/*
 * Sharded frames (SURVEY.md section 8(b), 8(e) mode 1): one process per GPU, RCCL point to point over xGMI, no collective.  Stands
 * behind `upscaler.enhance(img)` of standalone/direct_esrgan.py:148 (RealESRGANer(tile=512, tile_pad=10), :118-127) when one frame is
 * evaluated by several GPUs: the tiles of upstream's grid are independent network evaluations, dealt to the ranks in contiguous
 * runs balanced by padded area; the uint8 frame is row-scattered (rank r holds rows [r H / N, (r + 1) H / N)) and a rank fetches only
 * the rows its tiles read beyond its band; quantised tile centres are gathered on rank 0.
 *   nesr_comm_unique_id : rank 0 fills 128 bytes the host distributes by its own means (the launcher's rendezvous)
 *   nesr_comm_init      : every rank, with its rank / the world size / those 128 bytes (ncclCommInitRank on the context's device);
 *                         librccl.so is loaded on the first of these calls, never before
 *   nesr_forward_sharded_u8 : band_dev = this rank's rows of the u8 HWC BGR frame (device memory); out_dev (rank 0 only) = the
 *                         [H s, W s, 3] u8 BGR result; enqueued on hip_stream.  Without nesr_comm_init it is the one-rank case.
 *                         through_fp16 as in nesr_cut_tiles_u8 / nesr_paste_tiles_u8.  bf16 contexts only (NESR_ERR_ARG for any
 *                         other dtype, NESR_DTYPE_F16 included).
 *   nesr_shard_plan     : the plan by itself (host only, no device): tiles as 13 ints each (input window y0 y1 x0 x1, output window,
 *                         crop inside the tile's output, owner rank) and the row moves (src, dst, row lo, row hi); counts are always
 *                         returned, the arrays are filled when they are large enough.  `scale` = output / input size.
 */
int nesr_comm_unique_id(void* id128);
int nesr_comm_init(nesr_ctx* ctx, int rank, int nranks, const void* id128);
int nesr_comm_destroy(nesr_ctx* ctx);
int nesr_forward_sharded_u8(nesr_ctx* ctx, const uint8_t* band_dev, int H, int W, int tile, int tile_pad, int through_fp16, uint8_t* out_dev,
                            void* hip_stream);
int nesr_shard_plan(int H, int W, int scale, int tile, int tile_pad, int nranks, int* tiles13, int cap_tiles, int* ntiles, int* moves4,
                    int cap_moves, int* nmoves);

/*
 * the non-local means inside `cv2.fastNlMeansDenoisingColored(image, None, h, h, 7, 21)` of
 * SuperResolutionPipeline._preprocess_image (nesr/nesr.py:674), on [C, H, W] u8 planes taken as ONE C-channel image (C = 1: the L
 * plane, C = 2: the a and b planes).  weights_dev: int32 table over the binned ("almost", >> 6) template distance,
 * round(M exp(-d / (h^2 C))) with OpenCV's fixed-point M, 0 below M / 1000 (nesr_nl_means_weights or imgproc.nl_means_weights
 * builds it).  The Lab conversions around it: nesr_lab_u8; the whole pre-filter: nesr_preprocess_u8.  Parity unpinned against cv2
 * (absent): checked against oracle/cv2_ref.py, a restatement of OpenCV's invoker.
 */
int nesr_nl_means_u8(int device_id, const uint8_t* planes_dev, int C, int H, int W, int template_size, int search_size, const int* weights_dev, int nbins,
                     uint8_t* out_dev, void* hip_stream);

/*
 * `cv2.createCLAHE(clipLimit=2.0, tileGridSize=(8, 8)).apply(l)` of SuperResolutionPipeline._preprocess_image (nesr/nesr.py:680-684) on one
 * [H, W] u8 plane: per-tile clipped and redistributed histograms -> look-up tables (the image counts as padded by BORDER_REFLECT_101 to
 * a multiple of the grid -- both sides, only when one does not divide, as clahe.cpp does), every pixel the bilinear blend of the four
 * surrounding tiles' tables.  lut_dev: grid_x * grid_y * 256 floats of device scratch.  Bit for bit imgproc.clahe_u8's torch
 * composition; parity unpinned against cv2 (absent): checked against oracle/cv2_ref.py.
 */
int nesr_clahe_u8(int device_id, const uint8_t* gray_dev, int H, int W, double clip_limit, int grid_x, int grid_y, float* lut_dev, uint8_t* out_dev,
                  void* hip_stream);

/*
 * The rest of SuperResolutionPipeline._preprocess_image (nesr/nesr.py:668-689) and all of _postprocess_image (nesr/nesr.py:1056-1084)
 * as HIP kernels (csrc/filters.hip), for a host without torch.  Each entry is bit for bit the torch function of imgproc.py named
 * below (tests/test_gpu_filters_hip.py); parity against cv2 is unpinned (cv2 is absent): checked against oracle/cv2_ref.py, a
 * restatement of OpenCV's algorithms.  None of the argument checks touches a device; a bad argument returns NESR_ERR_ARG.
 *
 * nesr_lab_u8: cv2.cvtColor(COLOR_RGB2Lab | COLOR_Lab2RGB | COLOR_LBGR2Lab | COLOR_Lab2LBGR | ...) on u8 (L 255/100, a + 128,
 * b + 128) -- imgproc.rgb2lab_u8 / lab2rgb_u8; the reference calls them inside fastNlMeansDenoisingColored (nesr/nesr.py:674) and
 * around its CLAHE (nesr/nesr.py:680, 685).  mode = NESR_LAB_* bits: FROM_LAB (Lab -> RGB; else RGB -> Lab), LINEAR (no sRGB gamma),
 * FIRST_IS_BLUE (channel 0 is blue), PLANAR (the Lab side is [3, H, W] planes; the RGB side is always HWC).  src == dst is allowed
 * without PLANAR only.
 */
enum { NESR_LAB_FROM_LAB = 1, NESR_LAB_LINEAR = 2, NESR_LAB_FIRST_IS_BLUE = 4, NESR_LAB_PLANAR = 8 };
int nesr_lab_u8(int device_id, const uint8_t* src_dev, int H, int W, int mode, uint8_t* dst_dev, void* hip_stream);

/*
 * cv2.GaussianBlur(img, (ksize, ksize) or (0, 0), sigma) on [H, W, C] u8, C = 1 or 3 -- imgproc.gaussian_blur_u8, used twice by
 * _postprocess_image (nesr/nesr.py:1063, 1068): OpenCV's 8-bit fixed-point taps (nesr_gaussian_taps), a separable filter with int32
 * sums, BORDER_REFLECT_101, one rounding (v + 2^15) >> 16.  ksize 0 = round(6 sigma + 1) | 1; the kernel must be odd and at most
 * 31 taps.  src_dev != dst_dev.
 */
int nesr_gaussian_u8(int device_id, const uint8_t* src_dev, int H, int W, int C, double sigma, int ksize, uint8_t* dst_dev, void* hip_stream);

/* Host only: the integer taps of that blur -- imgproc.gaussian_kernel_u8 (OpenCV's tabulated small kernels for sigma <= 0, else the
 * sampled Gaussian normalised in double, x256 rounded, the centre tap making the sum 256).  *n is always set; taps[0 .. *n) is filled
 * when cap >= *n. */
int nesr_gaussian_taps(double sigma, int ksize, int* taps, int cap, int* n);

/* Host only: the weight table of nesr_nl_means_u8 for C channels and strength h -- imgproc.nl_means_weights (OpenCV's
 * almost_dist2weight, round(M exp(-d / (h^2 C))) with M = INT_MAX / (search^2 255), 0 below M / 1000, over bins of the template
 * distance >> shift).  *nbins and *shift are always set; table[0 .. *nbins) is filled when cap >= *nbins. */
int nesr_nl_means_weights(int C, double h, int template_size, int search_size, int* table, int cap, int* nbins, int* shift);

/*
 * _preprocess_image (nesr/nesr.py:668-689) on [H, W, 3] u8 RGB -- imgproc.preprocess_image: when denoise_level > 0,
 * fastNlMeansDenoisingColored(img, None, 10 denoise_level, 10 denoise_level, 7, 21) (LBGR -> Lab planes, nesr_nl_means_u8 on L and on
 * ab, Lab -> LBGR fused with the following RGB -> Lab); then CLAHE (clip 2.0, 8 x 8 tiles; nesr_clahe_u8) on L, Lab -> RGB.  All of it
 * is enqueued on hip_stream with no allocation, no synchronisation and no copy, except the first call for a (device, channels, h),
 * which builds the NL-means weight tables on the host and uploads them once (kept for the process).  scratch_dev: at least
 * nesr_preprocess_scratch_bytes(H, W) = 2 * round_up(3 H W, 256) + 65536 bytes of device memory.  rgb_dev == out_dev is allowed.
 */
size_t nesr_preprocess_scratch_bytes(int H, int W);
int nesr_preprocess_u8(int device_id, const uint8_t* rgb_dev, int H, int W, double denoise_level, void* scratch_dev, size_t scratch_bytes,
                       uint8_t* out_dev, void* hip_stream);

/*
 * _postprocess_image (nesr/nesr.py:1056-1084) on [H, W, 3] u8 RGB -- imgproc.postprocess_image: where the detail
 * saturate(gray - GaussianBlur(gray, sigma 2)) exceeds 10 the pixel becomes saturate(round(1.5 x - 0.5 GaussianBlur(x, sigma 3))),
 * elsewhere it stays; one launch.  adaptive_sharpening = 0: out = the input (a copy on hip_stream unless rgb_dev == out_dev).
 * rgb_dev != out_dev when sharpening.
 */
int nesr_postprocess_u8(int device_id, const uint8_t* rgb_dev, int H, int W, int adaptive_sharpening, uint8_t* out_dev, void* hip_stream);

/*
 * The image half of SuperResolutionPipeline._segment_and_enhance (nesr/nesr.py:726-747; standalone/superres_project.py:249-270) on
 * [H, W, 3] u8 RGB -- imgproc.segment_enhance.  Everything after the segmenter's argmax: mask_dev is `(seg_map > 0).astype(np.uint8)`
 * (nesr/nesr.py:731), [mask_h, mask_w] u8 {0, 1}, rows contiguous, at the segmenter's resolution.
 *   launch 1: `cv2.resize(object_mask, (w, h))` (:732, cv2's default INTER_LINEAR) = nesr_resize_cv_u8(NESR_INTER_LINEAR) into
 *             scratch_dev; skipped when the sizes are equal.  The rounded result is again {0, 1}.
 *   launch 2: one fused stencil -- `cv2.dilate(object_mask, np.ones((3, 3)))` (:735-736: the max over the neighbours inside the
 *             image; cv2's default border never wins a max), `cv2.GaussianBlur(enhanced, (0, 0), 3)` and
 *             `cv2.addWeighted(enhanced, 1.5, blurred, -0.5, 0)` (:739-740: saturate(round(1.5 x - 0.5 blur)), the value and the
 *             code of nesr_postprocess_u8), `np.where(mask == 1, sharpened, enhanced)` (:743-747).
 * scratch_dev: at least nesr_segment_enhance_scratch_bytes(H, W) = round_up(H W, 256) bytes of device memory, always required.
 * rgb_dev != out_dev.  Both launches are enqueued on hip_stream; no allocation and no synchronisation after the first call for a
 * (device, mask size, frame size), which uploads the mask's resize tables (as nesr_resize_cv_u8).  A null pointer, a size below 1,
 * rgb_dev == out_dev or a short scratch: NESR_ERR_ARG before any device is touched.
 * The reference's branch for frames above 1024 pixels (nesr/nesr.py:703-724) resizes the class map with INTER_NEAREST first;
 * nearest commutes with `> 0`, so a caller does it on the mask: nesr_resize_cv_u8(NESR_INTER_NEAREST) to H x W, then this entry.
 * Bit for bit imgproc.segment_enhance's torch chain; parity unpinned against cv2 (absent): checked against tests/cv2_stages_ref.py.
 */
size_t nesr_segment_enhance_scratch_bytes(int H, int W);
int nesr_segment_enhance_u8(int device_id, const uint8_t* rgb_dev, int H, int W, const uint8_t* mask_dev, int mask_h, int mask_w,
                            void* scratch_dev, size_t scratch_bytes, uint8_t* out_dev, void* hip_stream);

/*
 * SuperResolutionPipeline._ensemble_results (nesr/nesr.py:1033-1054) on 1 <= n <= 8 u8 images of equal shape [H, W, C], rows
 * contiguous; images_dev is a HOST array of n device pointers -- imgproc.ensemble_results after its Lanczos alignment.  The mean is
 * the arithmetic of nesr/nesr.py:1048-1054 under NumPy 1.x, every step rounded to float32: w = float32(1 / n), acc = 0, for each
 * image in order acc = fl32(acc + fl32(fl32(x) w)), truncated toward zero to u8 (for n <= 8, n copies of one image give it back:
 * float32(1 / n) is exact or rounded up; a mean of different images truncates, it does not round).
 * NumPy >= 2 would promote `img.astype(np.float32) * weights[i]` to float64 (the weight is a float64 scalar) and round once on the
 * `+=`; this library restates the NumPy 1.x result, the one the reference was written against.  n = 1 copies (nesr/nesr.py:1035-1036).
 * One elementwise launch on hip_stream that reads each input once, with 16-byte loads and stores when every pointer is 16-byte
 * aligned (one byte per thread otherwise); no allocation, no synchronisation.  n outside 1..8, a null pointer, a size below 1:
 * NESR_ERR_ARG before any device is touched.
 */
int nesr_ensemble_u8(int device_id, const uint8_t* const* images_dev, int n, int H, int W, int C, uint8_t* out_dev, void* hip_stream);

/*
 * cv2.imwrite(path, frame) for a .jpg / .jpeg path, the last call of every reference entry point (standalone/direct_esrgan.py:169,
 * nesr/nesr.py:646), as HIP kernels (csrc/jpeg.hip): the frame stays on the device and only the file crosses to the host.  cv2's
 * defaults: baseline JPEG, quality 95, 4:2:0 for colour, Annex K quantisation tables scaled by libjpeg's quality rule, Annex K
 * Huffman tables, libjpeg's islow integer FDCT, no restart markers, JFIF 1.01 header.  The integer pipeline is reproducible: the
 * bytes equal libjpeg-turbo's (pinned against Pillow's build of it in tests/test_jpeg_spec.py through tests/jpeg_ref.py, the
 * specification the kernels are compared with byte for byte; cv2 itself is absent).
 *
 * src_dev: [H, W, C] u8, C = 3 (order NESR_ORDER_RGB or NESR_ORDER_BGR: which channel comes first) or C = 1 (order ignored but
 * checked), pixels of a row contiguous, rows src_row_bytes apart; 1 <= H, W <= 65535; quality 1 .. 100.
 * scratch_dev: at least nesr_jpeg_scratch_bytes(H, W, C) bytes (0 for a shape it rejects), 16-byte aligned: about 350 bytes per
 * 8 x 8 block (coefficients, bit lengths, and an unstuffed stream sized for the worst case of 208 bytes per block).
 * out_dev[0 .. out_cap): the file.  out_len_dev (8-byte aligned): [0] = the bytes the whole file needs, [1] = 0 when it fits, 1 when
 * out_cap is smaller -- then out_dev holds the first out_cap bytes, nothing at or beyond out_cap is ever written, and a caller runs
 * again with out_cap >= [0] (or reports NESR_ERR_NOFIT).  Everything is enqueued on hip_stream: no allocation, no synchronisation, no
 * copy; two runs give the same bytes.  A null pointer, a size outside 1 .. 65535, C not 1 or 3, an unknown order, quality outside
 * 1 .. 100, a stride smaller than a row, a short or misaligned scratch: NESR_ERR_ARG before any device is touched.
 *
 * nesr_jpeg_header (host only): the bytes up to and including SOS -- SOI, APP0, DQT x 2 (x 1 for gray), SOF0, DHT x 4 (x 2), SOS: 623
 * bytes for colour, 328 for gray.  *n is always set; buf[0 .. *n) is filled when cap >= *n.
 */
enum { NESR_ORDER_RGB = 0, NESR_ORDER_BGR = 1 };
size_t nesr_jpeg_scratch_bytes(int H, int W, int C);
int nesr_jpeg_header(int H, int W, int C, int quality, uint8_t* buf, int cap, int* n);
int nesr_jpeg_encode_u8(int device_id, const uint8_t* src_dev, int64_t src_row_bytes, int H, int W, int C, int order, int quality, void* scratch_dev,
                        size_t scratch_bytes, uint8_t* out_dev, size_t out_cap, uint64_t* out_len_dev, void* hip_stream);

/*
 * The same encoder with libjpeg's other common settings -- cv2's IMWRITE_JPEG_SAMPLING_FACTOR, IMWRITE_JPEG_OPTIMIZE and
 * IMWRITE_JPEG_RST_INTERVAL -- byte for byte again (tests/jpeg_options_ref.py is the specification, pinned against Pillow's
 * libjpeg-turbo in tests/test_jpeg_options_spec.py).  The three entries above are these with {quality, NESR_JPEG_420, 0, 0}: the same
 * kernels, launches and bytes as before the options existed.
 *   sampling          NESR_JPEG_420 (cv2's default), NESR_JPEG_422 (h2v1: MCU Y0 Y1 Cb Cr, 16 x 8 pixels) or NESR_JPEG_444 (MCU
 *                     Y Cb Cr, 8 x 8 pixels); a gray frame ignores it.  4:4:0 and 4:1:1 are not encoded.
 *   optimize          non-zero: Huffman tables built for the frame (libjpeg's jpeg_gen_optimal_table) on the device, from
 *                     histograms taken on the device.  The DHT segments' lengths depend on the frame, so the header's length is known
 *                     on the device only: nesr_jpeg_header_ex refuses (NESR_ERR_ARG), the length word [0] counts it as always.
 *                     Byte parity with libjpeg is claimed for frames of up to 500 Mpixel (22360 x 22360): libjpeg's table
 *                     builder never picks a symbol or subtree counted more than 10^9 times, which no table of such a frame
 *                     reaches (at most 126 chroma AC symbols per 64 pixels at 4:4:4).  A larger frame still gets a valid file
 *                     with the true Huffman code of its counts, which libjpeg's own file then need not equal.
 *   restart_interval  MCUs per restart interval, 0 (none) .. 65535: DRI behind the DHTs, predictors back at 0 and the stream padded
 *                     to a byte at each interval's end, FF D0 .. FF D7 in turn between intervals.  Such a file is decoded one
 *                     interval per lane by nesr_jpeg_decode_u8, without its synchronisation rounds.
 * The scratch grows by 10 KiB with optimize and by 17 bytes per interval with a restart interval: nesr_jpeg_scratch_bytes_ex.
 * Capacity, the length and status words and the argument checks are nesr_jpeg_encode_u8's; null options, a sampling outside the three
 * or an interval outside 0 .. 65535: NESR_ERR_ARG before any device is touched.
 */
enum { NESR_JPEG_420 = 0, NESR_JPEG_422 = 1, NESR_JPEG_444 = 2 };
typedef struct nesr_jpeg_opts {
    int32_t quality, sampling, optimize, restart_interval;
} nesr_jpeg_opts;
size_t nesr_jpeg_scratch_bytes_ex(int H, int W, int C, const nesr_jpeg_opts* opts);
int nesr_jpeg_header_ex(int H, int W, int C, const nesr_jpeg_opts* opts, uint8_t* buf, int cap, int* n);
int nesr_jpeg_encode_ex_u8(int device_id, const uint8_t* src_dev, int64_t src_row_bytes, int H, int W, int C, int order, const nesr_jpeg_opts* opts,
                           void* scratch_dev, size_t scratch_bytes, uint8_t* out_dev, size_t out_cap, uint64_t* out_len_dev, void* hip_stream);

/*
 * cv2.imread(path) for a .jpg / .jpeg path, the first call of every reference entry point (nesr/nesr.py:661-666,
 * standalone/direct_esrgan.py:130), as HIP kernels (csrc/jpeg_decode.hip): the file's bytes go up, a tenth of the frame, and the
 * frame is born on the device.  libjpeg-turbo's default decompressor (JDCT_ISLOW, fancy upsampling, no merged upsampling) pixel for
 * pixel (tests/jpeg_decode_ref.py is the specification, pinned against Pillow's build of the library in
 * tests/test_jpeg_decode_spec.py).  EXIF orientation is not applied: that is cv2.IMREAD_UNCHANGED's behaviour, and a gray file gives
 * one channel as it does there.
 *
 * Supported: SOF0 / SOF1 Huffman, 8 bits, one interleaved scan over all components, 1 component or 3 (YCbCr), sampling 1x1 gray,
 * 4:4:4, 4:2:2 (h2v1), 4:2:0 (h2v2), 8-bit DQT, any DHT, any DRI; APPn and COM are skipped.  A valid file outside that list
 * (progressive, arithmetic, 12 bits, 4 components, Adobe transform 0, other sampling, several scans, 16-bit DQT) is
 * NESR_ERR_UNSUPPORTED; malformed segments are NESR_ERR_BADFILE.
 *
 * nesr_jpeg_parse (host only; replaces the header half of cv2.imread): walks the marker segments of file[0 .. n) up to SOS and fills
 * *info; it never reads the scan.  The Huffman tables are resolved per component (dc[c], ac[c] are the tables component c's scan
 * selector names) as decode look-up tables: look[next 9 bits] = length << 8 | symbol for codes of at most 9 bits (0 otherwise), and
 * libjpeg's maxcode / valoff / vals for the longer ones.  q[c]: component c's quantisation table in natural order.  hs, vs: the luma
 * sampling factors (1, 1 for gray, whose scan is not interleaved).
 *
 * nesr_jpeg_decode_u8 (replaces the decoding half of cv2.imread): file_dev[0 .. n) is the whole file on the device, info what
 * nesr_jpeg_parse gave for it.  dst_dev: [H, W, C] u8, rows dst_row_bytes apart, order NESR_ORDER_RGB or NESR_ORDER_BGR (C = 1:
 * [H, W]); bytes between the rows are not written.  scratch_dev: at least nesr_jpeg_decode_scratch_bytes(info) bytes, 16-byte
 * aligned.  status_dev (4-byte aligned): 0 when the scan decoded, otherwise bits that say why the device rejected it (a code that is
 * not in the table, a run past coefficient 63, a stream that ends early, more blocks than the frame holds, a wrong restart marker);
 * a caller reports NESR_ERR_BADFILE then, and dst_dev holds no defined image.  Every loop of the kernels is bounded by the stream's
 * length and the frame's block count and every store is guarded, so a corrupt scan ends in that word.  What libjpeg would recover
 * from such a file is not reproduced.  With a restart interval everything is enqueued on hip_stream and nothing waits; without one
 * the self-synchronising decode launches its cross-workgroup pass until a 4-byte count it reads back is zero (at most once per
 * workgroup of 256 x 1024 bits, usually twice).  A null pointer, an info that does not describe file[0 .. n), an unknown order, a
 * stride smaller than a row, a short or misaligned scratch: NESR_ERR_ARG before any device is touched.
 */
typedef struct nesr_jpeg_huff {
    uint16_t look[512];
    int32_t maxcode[18]; /* [l]: the largest code of length l, -1 when there is none; [17] ends every search */
    int32_t valoff[17];  /* vals[code + valoff[l]] */
    uint8_t vals[256];
} nesr_jpeg_huff;
typedef struct nesr_jpeg_info {
    int32_t H, W, C;
    int32_t hs, vs;
    int32_t restart_interval; /* MCUs, 0: none */
    int32_t mcus_x, mcus_y;
    int64_t scan_offset, scan_bytes; /* the entropy-coded bytes: after SOS, up to EOI when the file ends with one */
    uint16_t q[3][64];
    nesr_jpeg_huff dc[3], ac[3];
} nesr_jpeg_info;
int nesr_jpeg_parse(const uint8_t* file, size_t n, nesr_jpeg_info* info);
size_t nesr_jpeg_decode_scratch_bytes(const nesr_jpeg_info* info);
int nesr_jpeg_decode_u8(int device_id, const uint8_t* file_dev, size_t n, const nesr_jpeg_info* info, uint8_t* dst_dev, int64_t dst_row_bytes, int order,
                        void* scratch_dev, size_t scratch_bytes, uint32_t* status_dev, void* hip_stream);
/* What this thread's last nesr_jpeg_decode_u8 enqueued: launches of the cross-workgroup synchronisation pass (0 with a restart
 * interval or a stream of one workgroup) and kernel launches in all.  For measurements (tools/bench_jpeg_decode.py). */
int nesr_jpeg_decode_last_launches(int* sync_rounds, int* launches);

/*
 * cv2.imwrite(path, frame) for a .png path as HIP kernels (csrc/png.hip): the lossless file, which is the one the reference writes
 * most -- standalone/superres_project.py:203-206 always names its result .png, nesr/nesr.py:619-625 saves intermediate_iter{n}.png
 * after every iteration, and standalone/direct_esrgan.py:130,169 reads with IMREAD_UNCHANGED and writes with the input's extension,
 * so a PNG with alpha, a gray scan or a 16-bit file comes back as PNG (the BGRA, 16-bit gray and 16-bit colour frames nesr_pack_frame
 * takes).  The frame stays on the device and only the file crosses to the host.
 *
 * Lossless is the contract: a standard decoder returns the frame bit for bit.  The bytes are NOT cv2's (zlib's LZ77 output depends
 * on its version); they are those of tests/png_ref.py, the specification the kernels are compared with byte for byte: signature,
 * IHDR (depth 8 or 16; colour type 0, 2 or 6; no interlace), IDAT[78 01], one IDAT per deflate chunk, IDAT[Adler-32], IEND, no
 * ancillary chunk.  Per row the cheapest of the five filter types by libpng's sum of min(v, 256 - v), each computed from raw
 * neighbours; the filtered stream is cut into chunks of 32768 bytes, each one deflate block (stored, fixed or dynamic, the cheapest by
 * exact bit count) with distance-1 matches only, followed by an empty stored block that re-aligns the stream (pigz's scheme).
 *
 * src_dev: [H, W, C] samples of `depth` bits (8: bytes; 16: little-endian 16-bit words, as nesr_unpack_frame leaves them), C = 1, 3
 * or 4, order NESR_ORDER_RGB or NESR_ORDER_BGR (which channel comes first; the file is always R G B (A); C = 1: ignored but checked),
 * pixels of a row contiguous, rows src_row_bytes apart; 1 <= H, W <= 65535.
 * scratch_dev: at least nesr_png_scratch_bytes(H, W, C, depth) bytes (0 for a shape it rejects), 16-byte aligned: the filtered
 * stream and one 32800-byte slot per chunk, about twice the frame.
 * out_dev[0 .. out_cap): the file; nesr_png_bound(H, W, C, depth) is the exact worst case (every chunk stored: 75 bytes, the
 * filtered stream and 22 bytes per chunk), so a buffer of that size always fits.  out_len_dev (8-byte aligned): [0] = the bytes the
 * whole file needs, [1] = 0 when it fits, 1 when out_cap is smaller -- then out_dev holds the first out_cap bytes, nothing at or
 * beyond out_cap is ever written, and a caller reports NESR_ERR_NOFIT.  Everything is enqueued on hip_stream: no allocation, no
 * synchronisation, no copy; two runs give the same bytes.  A null pointer, a size outside 1 .. 65535, C not 1, 3 or 4, depth not 8 or
 * 16, an unknown order, a stride smaller than a row, a short or misaligned scratch: NESR_ERR_ARG before any device is touched.
 *
 * nesr_png_head (host only): signature, IHDR and the 2-byte IDAT that holds the zlib header, 47 bytes.  *n is always set;
 * buf[0 .. *n) is filled when cap >= *n.
 * nesr_png_code_lengths (host only): the code-length construction the kernels run per chunk (png_ref.code_lengths), for tests: a
 * length-limited Huffman code for counts[0 .. n), 2 <= n <= 286, n <= 2^limit, limit <= 15, counts summing to less than 2^32.  The code
 * is always complete: with fewer than two counted symbols that symbol (or symbol 0) and the lowest other one get one bit.
 */
size_t nesr_png_bound(int H, int W, int C, int depth);
size_t nesr_png_scratch_bytes(int H, int W, int C, int depth);
int nesr_png_head(int H, int W, int C, int depth, uint8_t* buf, int cap, int* n);
int nesr_png_code_lengths(const uint32_t* counts, int n, int limit, uint8_t* lengths);
int nesr_png_encode(int device_id, const void* src_dev, int64_t src_row_bytes, int H, int W, int C, int depth, int order, void* scratch_dev,
                    size_t scratch_bytes, uint8_t* out_dev, size_t out_cap, uint64_t* out_len_dev, void* hip_stream);

/*
 * cv2.imread(path.png, cv2.IMREAD_UNCHANGED) as HIP kernels (csrc/png_decode.hip): the way gray, BGRA and 16-bit frames arrive
 * (standalone/direct_esrgan.py:130), and the way a run reads what the run before it wrote.  tests/png_decode_ref.py is the
 * specification.  Supported: depth 8 or 16, colour type 0, 2 or 6, no interlace, at most 65535 x 65535 (C = 1, 3 or 4).  Palette,
 * gray + alpha, depth 1 / 2 / 4, Adam7: NESR_ERR_UNSUPPORTED.  A malformed file, or a zlib header with CM != 8, a window above 32 KiB,
 * FDICT set or a bad check value: NESR_ERR_BADFILE.
 *
 * nesr_png_parse (host only, never reads at or beyond file + n): the signature; the chunk walk with every length checked; IHDR first,
 * its CRC checked; IDATs consecutive and at least one; ancillary chunks and PLTE skipped; IEND last.  The CRCs of the other chunks are
 * not checked: the decoder checks the Adler-32 of the inflated stream instead.  It fills info and the segment plan: with Z the IDAT
 * payloads joined and D = Z[2 : -4] the deflate stream, a cut is an IDAT boundary strictly inside D whose preceding four bytes of D
 * are 00 00 FF FF (the empty stored block of a flush), and a segment is the D-bytes between two cuts -- offset: where its first byte
 * lies in the file, bytes, first, last.  info->contiguous: no segment spans an IDAT boundary, so segment i is file[offset .. offset +
 * bytes); only such a plan goes to nesr_png_decode.  A file of nesr_png_encode gives one segment per 32 KiB chunk.  segs[0 .. cap)
 * receives the first cap segments (segs may be null when cap is 0); info->n_segments is set even when cap is smaller, and the call
 * then returns NESR_ERR_NOFIT: size the table and call again.
 *
 * nesr_png_decode: file_dev[0 .. n) the file on the device, segs_dev the info->n_segments segments on the device (8-byte aligned).
 * Each segment is inflated alone by one wave -- a measuring pass, a scan of the sizes, a writing pass -- then the Adler-32 is checked
 * and the row filters are undone.  dst_dev: [H, W, C] samples (8 bit: bytes; 16 bit: little-endian words, as nesr_pack_frame takes
 * them), order NESR_ORDER_RGB or NESR_ORDER_BGR (alpha last; C = 1: ignored but checked), rows dst_row_bytes apart, nothing between
 * the rows is written.  scratch_dev: nesr_png_decode_scratch_bytes(info) bytes (0 for an info it rejects), 16-byte aligned, about
 * twice the frame.  *status_dev (4-byte aligned) is 0 after a good decode, else a set of bits, and dst_dev holds no defined image:
 *   1 a segment's input ran out   2 a code that is in no table, or symbol 286 / 287 / distance 30 / 31   4 LEN != ~NLEN
 *   8 BTYPE 3 or a broken dynamic header   16 DEPENDENT: a distance that reaches before its segment (a Z_SYNC_FLUSH file; inflate
 *   it on the host)   32 BFINAL before the last segment, or bytes behind the last block   64 the sizes do not add up to
 *   H (1 + W bpp)   128 the Adler-32   256 a filter type above 4
 * A caller reports NESR_ERR_BADFILE for every bit but 16.  No kernel loads beyond n or stores beyond what it was given, whatever the
 * file holds; a pass that finds the word non-zero does nothing.  Everything is enqueued on hip_stream: no allocation, no
 * synchronisation, no copy.
 *
 * nesr_png_unfilter: the second half alone, for a stream the host inflated (a file of one deflate stream): filtered_dev holds the
 * H (1 + W bpp) bytes of the filtered stream; scratch_dev: nesr_png_unfilter_scratch_bytes(H, W, C, depth) bytes.  *status_dev: 0 or 256.
 *
 * A null pointer, an info or shape outside the list above, a plan that is not contiguous, an unknown order, a stride smaller than a
 * row, a short or misaligned scratch: NESR_ERR_ARG before any device is touched.
 */
typedef struct nesr_png_segment {
    int64_t offset, bytes;
    int32_t first, last;
} nesr_png_segment;
typedef struct nesr_png_info {
    int32_t H, W, C, depth, contiguous, n_segments;
    int64_t stream_bytes;                  /* H (1 + W bpp) */
    uint32_t adler;                        /* the file's Adler-32 of the filtered stream */
} nesr_png_info;
int nesr_png_parse(const uint8_t* file, size_t n, nesr_png_info* info, nesr_png_segment* segs, int cap);
size_t nesr_png_decode_scratch_bytes(const nesr_png_info* info);
int nesr_png_decode(int device_id, const uint8_t* file_dev, size_t n, const nesr_png_info* info, const nesr_png_segment* segs_dev, void* dst_dev,
                    int64_t dst_row_bytes, int order, void* scratch_dev, size_t scratch_bytes, uint32_t* status_dev, void* hip_stream);
size_t nesr_png_unfilter_scratch_bytes(int H, int W, int C, int depth);
int nesr_png_unfilter(int device_id, const uint8_t* filtered_dev, int H, int W, int C, int depth, void* dst_dev, int64_t dst_row_bytes, int order,
                      void* scratch_dev, size_t scratch_bytes, uint32_t* status_dev, void* hip_stream);

/*
 * cv2.resize as HIP kernels (csrc/resize.hip), for a host without torch: upstream's `cv2.resize(output, ..., INTER_LANCZOS4)` behind
 * RealESRGANer.enhance(outscale=...), its `cv2.resize(alpha, ..., INTER_LINEAR)` behind alpha_upsampler != "realesrgan", and the
 * Lanczos paste of _process_with_tiling (nesr/nesr.py:437-446).  cv2's semantics as imgproc.lanczos4_resize / linear_resize_f32 and
 * oracle/cv2_ref.py restate them: sampling position (d + 0.5) n_in / n_out - 0.5 in double, cast to float32, floor + fraction;
 * Lanczos-4 always takes 8 taps from floor - 3 (also when shrinking), source indices clamped (BORDER_REPLICATE).  Three forms:
 *   nesr_resize_u8   NESR_INTER_LANCZOS4, C = 1, 3, 4: OpenCV's fixed point -- coefficients short(rint(c 2048)), integer horizontal
 *                    pass, integer vertical pass, (v + 2^21) >> 22, saturate.  Bit for bit imgproc.lanczos4_resize's torch chain.
 *   nesr_resize_u16  NESR_INTER_LANCZOS4, C = 1, 3, 4: float32 coefficients, per pass acc = acc + w_k x_k with k ascending, product and
 *                    sum rounded separately, rint, saturate.  Bit for bit oracle/cv2_ref.py; the torch chain sums in torch's order (+-1).
 *   nesr_resize_f32  NESR_INTER_LINEAR, C = 1 .. 4: a (1 - f) + b f per pass, every operation rounded by itself, f = 0 at the clamped
 *                    ends.  Bit for bit imgproc.linear_resize_f32's torch chain.
 * Any other (type, interp) pair, a null pointer, a size below 1, another channel count, a row stride smaller than the row,
 * src == dst, or (u16, f32) a pointer or stride that is not a multiple of the sample size: NESR_ERR_ARG, before any device is
 * touched.  Equal sizes are legal and copy the image.
 *
 * Images are HWC with the pixels of a row contiguous, addressed as base pointer + row stride in BYTES: a rectangle of a frame is
 * the pointer to its first pixel with the frame's stride -- crop, resize and paste into a rectangle of a canvas are one call.  The
 * rectangle is its own image (the border is the rectangle's edge), and no byte of the destination outside dst_h x dst_w x C is
 * written.  The Lanczos forms are one launch: both passes, no intermediate in device memory.
 *
 * The coefficient tables are built on the host (nesr_resize_taps gives the same values) and kept on the device per
 * (device, kind, n_in, n_out): the first call for an axis pair allocates and uploads (synchronous); every later call with those
 * sizes allocates nothing, does not synchronise, and only enqueues on hip_stream.  Any thread may call.
 * Parity unpinned against cv2 (absent): checked against oracle/cv2_ref.py.
 */
enum { NESR_INTER_LINEAR = 1, NESR_INTER_LANCZOS4 = 4 };   /* cv2's values */
int nesr_resize_u8(int device_id, const uint8_t* src_dev, int src_h, int src_w, int C, int64_t src_row_bytes, uint8_t* dst_dev, int dst_h, int dst_w,
                   int64_t dst_row_bytes, int interp, void* hip_stream);
int nesr_resize_u16(int device_id, const uint16_t* src_dev, int src_h, int src_w, int C, int64_t src_row_bytes, uint16_t* dst_dev, int dst_h, int dst_w,
                    int64_t dst_row_bytes, int interp, void* hip_stream);
int nesr_resize_f32(int device_id, const float* src_dev, int src_h, int src_w, int C, int64_t src_row_bytes, float* dst_dev, int dst_h, int dst_w,
                    int64_t dst_row_bytes, int interp, void* hip_stream);

/* Host only: the table of one axis resized n_in -> n_out.  *n_out_written = n_out always; the arrays are filled when both are given
 * and cap (in positions) >= n_out.
 *   NESR_INTER_LANCZOS4: first_out[d] = floor(position) - 3, the first of the 8 taps, NOT clamped (the kernels clamp every tap to
 *     [0, n_in - 1]); coef_out[16 d .. 16 d + 8) = the float32 coefficients (the u16 form), coef_out[16 d + 8 .. 16 d + 16) = the
 *     11-bit fixed-point coefficients short(rint(c 2048)) as floats (the u8 form; they sum to 2048 up to rounding).
 *   NESR_INTER_LINEAR: first_out[d] = the clamped first index i0; coef_out[2 d] = f (0 at the clamped ends), coef_out[2 d + 1] =
 *     i1 - i0 (1, or 0 at the last sample). */
int nesr_resize_taps(int n_in, int n_out, int interp, int* first_out, float* coef_out, int cap, int* n_out_written);

/*
 * 8-bit cv2.resize with cv2's other interpolations (csrc/resize.hip) -- imgproc.resize_u8: the bicubic step the loop takes when no
 * model contributes (nesr/nesr.py:597-605; also downsample_image's default, nesr/utils/image_utils.py:119-128), the default
 * (linear) resize of the object mask (nesr/nesr.py:732) and the nearest resize of the class map (nesr/nesr.py:720-724).  The
 * contract is nesr_resize_u8's: C = 1, 3 or 4; base pointer + row stride in bytes, no byte outside the destination rectangle is
 * written; equal sizes copy; every argument is checked before a device is touched (an interp that is none of the four, C = 2, a
 * null pointer, a short stride, src == dst: NESR_ERR_ARG); tables per (device, kind, n_in, n_out), later calls only enqueue.  Each
 * form is one launch with both passes and no intermediate in device memory.  The sampling position is nesr_resize_u8's:
 * (d + 0.5) n_in / n_out - 0.5 in double, cast to float32, floor + fraction f.  The arithmetic is OpenCV 4.x resize.cpp's:
 *   NESR_INTER_NEAREST   source index min(floor(d n_in / n_out), n_in - 1) per axis (the product in double); samples are copied.
 *   NESR_INTER_LINEAR    taps (s, s + 1); f = 0 and s clamped when s < 0 or s >= n_in - 1; coefficients short(rint((1 - f) 2048)) and
 *                        short(rint(f 2048)), 1 - f in float32; horizontal t = S[s] a0 + S[s + 1] a1 in int32; vertical
 *                        (((b0 (t0 >> 4)) >> 16) + ((b1 (t1 >> 4)) >> 16) + 2) >> 2.  When BOTH axes shrink by exactly 2 cv2 takes its
 *                        area filter instead: (a + b + c + d + 2) >> 2 over the 2 x 2 block.
 *   NESR_INTER_CUBIC     4 taps from s - 1, indices clamped to [0, n_in - 1], f NOT zeroed at the ends; Keys weights with A = -0.75 in
 *                        float32, evaluated left to right: w0 = ((A (f + 1) - 5 A)(f + 1) + 8 A)(f + 1) - 4 A,
 *                        w1 = ((A + 2) f - (A + 3)) f f + 1, w2 = the same in 1 - f, w3 = 1 - w0 - w1 - w2; each short(rint(w 2048));
 *                        integer horizontal and vertical sums, (v + 2^21) >> 22, saturated (the Lanczos kernel with 4 taps).
 *   NESR_INTER_LANCZOS4  forwards to nesr_resize_u8: the same bytes.
 * Bit for bit imgproc.resize_u8's torch chain; parity unpinned against cv2 (absent): checked against tests/cv2_stages_ref.py.
 *
 * nesr_resize_cv_taps (host only): the integer table of one axis as the kernels read it.  *n_out_written = n_out always; the arrays
 * are filled when both are given and cap (in positions) >= n_out.  first_out[d], then per position in coef_out:
 *   NESR_INTER_NEAREST   first = the source index;                      1 coefficient:  1
 *   NESR_INTER_LINEAR    first = s, clamped (second tap min(s + 1, n_in - 1)); 2 coefficients: a0, a1 (they sum to 2048)
 *   NESR_INTER_CUBIC     first = floor(position) - 1, NOT clamped;      4 coefficients: coef_out[4 d .. 4 d + 4)
 *   NESR_INTER_LANCZOS4  first = floor(position) - 3, NOT clamped;      8 coefficients: coef_out[8 d .. 8 d + 8)
 */
enum { NESR_INTER_NEAREST = 0, NESR_INTER_CUBIC = 2 };   /* cv2's values, beside NESR_INTER_LINEAR and NESR_INTER_LANCZOS4 */
int nesr_resize_cv_u8(int device_id, const uint8_t* src_dev, int src_h, int src_w, int C, int64_t src_row_bytes, uint8_t* dst_dev, int dst_h, int dst_w,
                      int64_t dst_row_bytes, int interp, void* hip_stream);
int nesr_resize_cv_taps(int n_in, int n_out, int interp, int* first_out, int* coef_out, int cap, int* n_out_written);

/*
 * Gray, BGRA and 16-bit frames (csrc/frame_io.hip): every kind of frame RealESRGANer.enhance (realesrgan utils.py) takes besides
 * 8-bit BGR, which has nesr_forward_u8 -- behind `upscaler.enhance(img)` of standalone/direct_esrgan.py:148 and
 * standalone/superres_project.py:282 when the file read was a 16-bit TIFF, a gray scan or a PNG with alpha.
 *
 * nesr_pack_frame replaces enhance()'s host preparation: `img = img.astype(np.float32)`, `img / max_range`, for a gray frame
 * `cv2.cvtColor(img, cv2.COLOR_GRAY2RGB)`, for colour `cv2.cvtColor(img, cv2.COLOR_BGR2RGB)`, and pre_process's HWC -> CHW.
 *   src_dev      : [H, W] (channels 1) or [H, W, channels] (3 = BGR, 4 = BGRA) samples of `bits` bits (8: uint8, 16: uint16), the
 *                  samples of a row contiguous, rows src_row_bytes apart
 *   max_range    : 255 or 65535 -- what enhance() divides by (65535 when the frame's maximum exceeds 256, else 255: a uint16 frame
 *                  that dark counts as 8-bit range and comes back as uint8); the division is correctly rounded
 *   through_fp16 : as nesr_cut_tiles_u8 (RealESRGANer(half=True): `self.img = self.img.half()`)
 *   image_dev    : [1, 3, H, W] f32, gray replicated, colour flipped to RGB -- what nesr_forward takes
 *   alpha_dev    : channels 4 only, may be null (alpha is not written).  NESR_ALPHA_NETWORK: [1, 3, H, W] f32, the alpha samples
 *                  replicated (`cv2.cvtColor(alpha, cv2.COLOR_GRAY2RGB)`), for a second nesr_forward; NESR_ALPHA_LINEAR: [H, W] f32
 *                  (never through fp16: it does not pass the network), for nesr_resize_f32
 *
 * nesr_unpack_frame replaces what enhance() does with the network's output: `.float().cpu().clamp_(0, 1)`, `[[2, 1, 0]]` and
 * CHW -> HWC, `cv2.cvtColor(output, cv2.COLOR_BGR2GRAY)` for a gray frame and for a network-upsampled alpha (0.114 b + 0.587 g +
 * 0.299 r, each product and sum rounded to float32 by itself, left to right), the concatenation of the alpha channel, and
 * `(output * max_range).round().astype(np.uint8 | np.uint16)` (round half to even).
 *   image_dev    : the network's output, [3] f32 planes image_plane floats apart, rows image_row floats apart -- post_process's
 *                  cropped view of a larger output is read in place
 *   alpha_dev    : channels 4 only.  NESR_ALPHA_NETWORK: the alpha pass's output, planes and rows alpha_plane / alpha_row floats
 *                  apart; NESR_ALPHA_LINEAR: one [Ho, Wo] f32 plane, rows alpha_row floats apart (clamped like the rest, not
 *                  rounded through fp16)
 *   dst_dev      : [Ho, Wo] (channels 1) or [Ho, Wo, channels] samples of `bits` bits, rows dst_row_bytes apart
 * Both are one launch on hip_stream, no allocation, no synchronisation; bit for bit frame_io.py's torch chains, which are the
 * numpy lines above.  channels not 1, 3 or 4, bits not 8 or 16, max_range not 255 or 65535, 65535 with 8 bits, a null pointer, a
 * size below 1, a pitch smaller than a row, or a uint16 pointer or pitch that is odd: NESR_ERR_ARG, before any device is touched.
 *
 * nesr_enhance_frame is enhance() for one untiled frame on one context, RRDBNet or SRVGGNetCompact: nesr_pack_frame,
 * nesr_forward, for BGRA either a second nesr_forward on the alpha planes (NESR_ALPHA_NETWORK, enhance's
 * alpha_upsampler="realesrgan") or nesr_resize_f32 of the alpha plane (NESR_ALPHA_LINEAR: upstream's
 * `cv2.resize(alpha, (w * scale, h * scale), interpolation=cv2.INTER_LINEAR)`, parity unpinned as everywhere), nesr_unpack_frame.
 *   src_dev  : as nesr_pack_frame, rows contiguous;  dst_dev : the frame s times the size (s = the context's output / input size),
 *              channels as src, uint8 when max_range is 255 and uint16 when it is 65535, rows contiguous
 *   scratch_dev : at least nesr_frame_scratch_bytes(ctx, H, W, channels, alpha_mode) bytes of device memory, 256-byte aligned (the
 *              float planes between the steps); 0 is returned for arguments nesr_enhance_frame would refuse
 * H and W must be multiples of the network's unshuffle factor (RealESRGANer pads a frame that is not; a C host pads before the
 * call), the network 3 channels in and out.  Those, every error of nesr_pack_frame, an alpha_mode that is neither constant and
 * scratch that is null or too small: NESR_ERR_ARG before any device is touched.  Call nesr_check_range before trusting dst_dev, as
 * after nesr_forward.
 */
enum { NESR_ALPHA_NETWORK = 0, NESR_ALPHA_LINEAR = 1 };
int nesr_pack_frame(int device_id, const void* src_dev, int H, int W, int channels, int bits, int64_t src_row_bytes, int max_range, int through_fp16,
                    float* image_dev, int alpha_mode, float* alpha_dev, void* hip_stream);
int nesr_unpack_frame(int device_id, const float* image_dev, int Ho, int Wo, int64_t image_plane, int64_t image_row, int through_fp16, int alpha_mode,
                      const float* alpha_dev, int64_t alpha_plane, int64_t alpha_row, int channels, int bits, int max_range, void* dst_dev,
                      int64_t dst_row_bytes, void* hip_stream);
size_t nesr_frame_scratch_bytes(const nesr_ctx* ctx, int H, int W, int channels, int alpha_mode);
int nesr_enhance_frame(nesr_ctx* ctx, const void* src_dev, int H, int W, int channels, int bits, int max_range, int alpha_mode, int through_fp16,
                       void* scratch_dev, size_t scratch_bytes, void* dst_dev, void* hip_stream);

/*
 * The ESRGAN stage of SuperResolutionPipeline.enhance_image (csrc/nesr12.hip, csrc/nesr_stage_api.cpp): the network the reference
 * builds and calls is RRDBNet(num_in_ch=12, num_out_ch=3, scale=4) (nesr/nesr.py:216), fed with a 12-channel synthesis of the RGB
 * frame and quantised by truncation.  With nesr_preprocess_u8 and nesr_postprocess_u8 one iteration of the pipeline is three calls on
 * device buffers; u8 frames go in and out, no float image exists outside the context's workspace.  Every entry is bit for bit the
 * torch statement in nesr_adapter.py named with it (tests/test_gpu_nesr_stage.py, tests/test_nesr_stage_host.py).
 *
 * nesr_forward_nesr_u8: _apply_esrgan_12channel (nesr/nesr.py:845-903; mode NESR_INPUT_12CH) or _apply_esrgan_3channel
 * (nesr/nesr.py:905-945; NESR_INPUT_3CH_X4) on one window -- nesr_adapter.apply_esrgan_12channel / apply_esrgan_3channel.
 *   rgb_dev : first pixel of an H x W window of an RGB u8 HWC frame, rows src_row_bytes apart.  The window is its own image: with
 *             bgr = the pixel flipped (cv2.COLOR_RGB2BGR) and t = bgr / 255 (correctly rounded), the network's input channels are
 *             t | clamp(1.1 t, 0, 1) | clamp(0.9 t, 0, 1) | cv2.GaussianBlur(bgr, (3, 3), 0) / 255 (taps [1 2 1] x [1 2 1], (S + 8) >> 4,
 *             BORDER_REFLECT_101 at the window's edges: the reference blurs a tile after cropping it), or t four times; one launch,
 *             written in the context's own activation layout
 *   out_dev : u8 RGB [4H, 4W, 3], rows out_row_bytes apart: clip(255 y, 0, 255) truncated (nesr/nesr.py:894-898), BGR -> RGB
 *             (:901), from conv_last's epilogue; rows further apart than 12 W bytes pass through the context's workspace
 * Requires an RRDBNet context with conv_first_in_ch 12, no unshuffle, num_out_ch 3, of any NESR_DTYPE_*; H, W >= 2 (for a
 * one-pixel side the torch statement pads by replication, not as cv2 does: not offered); strides at least a row.  Anything else,
 * an SRVGGNetCompact context included: NESR_ERR_ARG.  Call nesr_check_range before trusting out_dev, as after nesr_forward.
 *
 * nesr_stage_route (host only): the dispatch of _apply_esrgan (nesr/nesr.py:761-793) as nesr_adapter.apply_esrgan states it.
 * megapixels = H W / 1024^2; *tiled = enable_tiling and megapixels > threshold_mp (the reference's literals: 8 for cuda, 2 for cpu,
 * 4 for mps); *mode = NESR_INPUT_3CH_X4 if force_3channel else NESR_INPUT_12CH; megapixels > large_mp (the reference's literal 16)
 * forces tiling and NESR_INPUT_3CH_X4.
 *
 * nesr_stage_tile_plan (host only): the rectangles of _process_with_tiling (nesr/nesr.py:311-475) -- nesr_adapter.tile_plan.  Per
 * tile of the ceil(H / tile) x ceil(W / tile) grid, row-major, 13 ints:
 *     y0 y1 x0 x1      the source window, the tile grown by `padding` and clipped to the frame
 *     ty0 ty1 tx0 tx1  the crop inside the network's output of that window (net_scale times its size): int(padding scale) off every
 *                      side that is not a frame edge, clamped to at least one pixel
 *     oy0 oy1 ox0 ox1  the canvas rectangle: int(window edge x upscale_factor), moved in by int(padding upscale_factor) on the same sides
 *     skip             1: the rectangle is empty, nothing is pasted
 * in Python's arithmetic: doubles, int() truncating toward zero.  A crop whose size differs from its rectangle is resized into it
 * (Lanczos-4).  A frame that fits one tile (H <= tile and W <= tile) is one tile whose rectangle is the network's own output,
 * net_scale H x net_scale W, whatever upscale_factor says (nesr/nesr.py:326-328).  *n is always set; rects[0 .. 13 *n) is filled when
 * cap (in tiles) >= *n.
 *
 * nesr_apply_esrgan_u8: the stage -- nesr_adapter.apply_esrgan's two routes.  rgb_dev: u8 RGB [H, W, 3], rows contiguous.
 *   untiled (tiled = 0), or a frame that fits one tile: one nesr_forward_nesr_u8 into out_dev, u8 RGB [4H, 4W, 3]
 *   tiled: out_dev is the canvas, u8 RGB [int(H upscale_factor), int(W upscale_factor), 3], zeroed first; every tile of the plan
 *          runs through the network into scratch_dev, then its crop goes to its rectangle: a 2-D copy where the sizes agree, else
 *          nesr_resize_u8 (NESR_INTER_LANCZOS4) reading the crop in place and writing the rectangle in place
 * mode, tiled: nesr_stage_route's, or the caller's own.  padding: the reference passes 16 (nesr/nesr.py:797).  scratch_dev: at least
 * nesr_apply_esrgan_scratch_bytes(ctx, H, W, tiled, tile, padding) bytes (the largest tile's output; 256 where nothing is staged,
 * scratch_dev may be null then; 0 for arguments nesr_apply_esrgan_u8 would refuse).  Everything is enqueued on hip_stream; the call
 * allocates nothing and does not synchronise, except what nesr_forward and nesr_resize_u8 say of their first call for a size (the
 * workspace grows, a coefficient table is uploaded: nesr_reserve and one warm-up frame take both off the path).  Every refusal
 * (NESR_ERR_ARG: the context, a window side below 2, scratch) comes before the first launch.
 * ONE nesr_check_range after the call covers the whole frame: the range word is scoped to one forward, and every forward first moves
 * what the one before it left to the "earlier forward" word, which nesr_check_range reports as NESR_ERR_RANGE too -- a tile that did
 * not fit the compute form anywhere in the frame is an error for the frame.
 */
enum { NESR_INPUT_12CH = 0, NESR_INPUT_3CH_X4 = 1 };
int nesr_forward_nesr_u8(nesr_ctx* ctx, const uint8_t* rgb_dev, int64_t src_row_bytes, int H, int W, int mode, uint8_t* out_dev, int64_t out_row_bytes,
                         void* hip_stream);
int nesr_stage_route(int H, int W, int enable_tiling, int force_3channel, double threshold_mp, double large_mp, int* tiled, int* mode);
int nesr_stage_tile_plan(int H, int W, int tile, int padding, double upscale_factor, int net_scale, int* rects, int cap, int* n);
size_t nesr_apply_esrgan_scratch_bytes(const nesr_ctx* ctx, int H, int W, int tiled, int tile, int padding);
int nesr_apply_esrgan_u8(nesr_ctx* ctx, const uint8_t* rgb_dev, int H, int W, int mode, int tiled, int tile, int padding, double upscale_factor,
                         void* scratch_dev, size_t scratch_bytes, uint8_t* out_dev, void* hip_stream);

/*
 * Single-layer entry (test hook for the per-layer parity tests): one 3x3 stride-1 zero-pad-1
 * convolution + bias (+ LeakyReLU(0.2) if lrelu) (+ nearest x2 upsample of the input first if
 * upsample), i.e. torch.nn.Conv2d / F.leaky_relu / F.interpolate as composed in RRDBNet.forward.
 *   x_dev NCHW f32 [N,Cin,H,W];  w_host OIHW f32 [Cout,Cin,3,3];  b_host [Cout];
 *   y_dev NCHW f32 [N,Cout,H<<upsample,W<<upsample].  Synchronous.
 *   dtype NESR_DTYPE_F16: x and w are rounded to f16 (nearest even), the output passes through f16 storage; NESR_ERR_RANGE for
 *   a weight, input or output beyond +-65504.
 */
int nesr_conv3x3(int device_id, int dtype, const void* x_dev, int N, int Cin, int H, int W,
                 const float* w_host, const float* b_host, int Cout, int lrelu, int upsample,
                 void* y_dev, void* stream);
/* The same with the form of an upsampled NESR_DTYPE_F32_SPLIT layer chosen by hand (NESR_UPCONV_3X3 | NESR_UPCONV_2X2, see
 * nesr_set_upconv); nesr_conv3x3 takes the default (2x2 unless NESR_UPCONV=3x3).  Ignored where the folded form does not exist
 * (other dtypes, upsample = 0). */
int nesr_conv3x3_up(int device_id, int dtype, const void* x_dev, int N, int Cin, int H, int W,
                    const float* w_host, const float* b_host, int Cout, int lrelu, int upsample,
                    void* y_dev, void* stream, int upconv_mode);

/* Debug: the kernel family that the last nesr_conv3x3 / nesr_conv3x3_up call on the calling thread launched -- the decision its
 * launcher took, noted at the point of dispatch, not a second evaluation of the condition.  0 before any call on this thread and
 * after a call that failed before its launch.  A per-layer test asserts with it that it ran the kernel it is named after. */
enum { NESR_CONV_KERNEL_NONE = 0,
       NESR_CONV_KERNEL_GENERIC = 1,     /* conv3x3_mfma_kernel: f32 direct, and bf16 / f16 frames up to the size switch */
       NESR_CONV_KERNEL_XL = 2,          /* conv3x3_bf16_xl_kernel: the large-tile LDS-DMA kernel of bf16 / f16 */
       NESR_CONV_KERNEL_WINOGRAD = 3,    /* f32 Winograd F(2x2,3x3) */
       NESR_CONV_KERNEL_F16_PAIR = 4,    /* f32 as f16 pairs */
       NESR_CONV_KERNEL_UPCONV2X2 = 5 }; /* the folded 2x2-tap form of an upsampled f16-pair layer */
int nesr_debug_last_conv_kernel(void);

/*
 * ---- SegFormer, the pipeline's segmenter (csrc/segformer.hip, segformer_pre.hip, segformer_api.cpp) -- segformer.SegFormer.
 * `nvidia/segformer-b0-finetuned-ade-512-512`, which the reference's default configuration (segment_enhancement True,
 * nesr/nesr.py:40) loads at nesr/nesr.py:285-301 and runs on every iteration of enhance_image (:691-724).  f32 throughout, every
 * product on the f32-input MFMA; at most 80 kernel launches a frame at B0 (49 for a frame up to 1024 pixels, 51 above).
 *
 * nesr_segformer_create stands in for AutoModelForImageSegmentation.from_pretrained's construction (nesr/nesr.py:294-296): the
 * arrays hold num_encoder_blocks (1..4) entries each, named as SegformerConfig's fields.  Required: hidden_sizes[i] =
 * 32 num_attention_heads[i] (a head dimension of 32: B0; B1-B5 have 64), hidden sizes and decoder_hidden_size multiples of 32 up to
 * 256, 1 <= num_labels <= 256, num_channels 3.  The configuration is checked first: a bad one is NESR_ERR_ARG before any device is
 * touched.  LayerNorm eps 1e-5 (transformers builds every LayerNorm with torch's default, not config.layer_norm_eps), gelu (erf),
 * BatchNorm eps 1e-5 with its running statistics (eval mode).
 * nesr_segformer_load_weight stands in for its load_state_dict: a key is a transformers-5 name
 * (segformer.stages.{i}.blocks.{j}.attention.q_proj.weight ...) or the published checkpoint's transformers-4 name
 * (segformer.encoder.block.{i}.{j}.attention.self.query.weight ...), renamed here by the table of transformers'
 * conversion_mapping.py, so a C host loads the checkpoint as it is; data is host f32 in torch's layout, an unexpected key or a
 * wrong shape is NESR_ERR_ARG.
 * decode_head.batch_norm.num_batches_tracked is accepted and ignored.  nesr_segformer_num_tensors: the tensors finalize waits for
 * (207 at B0 with 150 labels).  nesr_segformer_finalize: a missing key is NESR_ERR_STATE; folds the BatchNorm into a scale and a
 * shift, transposes and uploads the weights.
 */
typedef struct nesr_segformer nesr_segformer;
int nesr_segformer_create(nesr_segformer** out, int device_id, int num_channels, int num_encoder_blocks, const int* depths,
                          const int* sr_ratios, const int* hidden_sizes, const int* patch_sizes, const int* strides,
                          const int* num_attention_heads, const int* mlp_ratios, int decoder_hidden_size, int num_labels);
void nesr_segformer_destroy(nesr_segformer* ctx);
int nesr_segformer_num_tensors(const nesr_segformer* ctx);
int nesr_segformer_load_weight(nesr_segformer* ctx, const char* key, const float* data_host, const int64_t* shape, int ndim);
int nesr_segformer_finalize(nesr_segformer* ctx);
/*
 * `outputs = model(pixel_values); outputs.logits` (nesr/nesr.py:713, 716): pixel_values_dev [1, 3, H, W] f32 -> logits_dev
 * [1, num_labels, oh, ow] f32, both on the context's device.  N must be 1, H and W multiples of 32 and H W <= 2^26
 * (NESR_ERR_ARG otherwise).
 * The entry takes no capacity: it writes num_labels * oh * ow floats, (oh, ow) being the first stage's token grid, which
 * nesr_segformer_output_size gives for the same patch_sizes, strides, H and W (H/4 x W/4 at B0's 7 x 7 / stride 4 patch embed;
 * every stage is a patch_sizes[i] x patch_sizes[i] conv of stride strides[i] with patch_sizes[i] / 2 padding).  The caller
 * sizes logits_dev by it.  nesr_segformer_output_size touches no device and needs no context.
 * Enqueued on hip_stream; the workspace grows on the first call for a larger size (that call synchronises the device).
 */
int nesr_segformer_output_size(int num_encoder_blocks, const int* patch_sizes, const int* strides, int H, int W, int* out_h, int* out_w);
int nesr_segformer_forward_f32(nesr_segformer* ctx, const float* pixel_values_dev, int N, int C, int H, int W, float* logits_dev,
                               void* hip_stream);
/*
 * nesr/nesr.py:701-716 on an [H, W, 3] u8 RGB frame on the device: `pil_image.resize(new_size, Image.LANCZOS)` when
 * max(W, H) > 1024 (new_size = (int(W s), int(H s)), s = 1024 / max(W, H)), the extractor's resize to 512 x 512 (PIL BILINEAR) and
 * normalisation ((v / 255 - mean) / std, ImageNet's), the network, `logits.argmax(dim=1)` at the logits' own size: class_map_dev
 * [oh, ow] u8 with (oh, ow) = nesr_segformer_output_size(..., 512, 512): 128 x 128 at B0 (capacity: the bytes class_map_dev holds,
 * at least oh * ow, NESR_ERR_ARG otherwise), *out_h = oh, *out_w = ow.  The lowest class wins a tie; the logits are never
 * written to memory.  The map's resize back to the frame (:719-724) is the caller's, on the mask (see nesr_segment_enhance_u8).
 * nesr_segformer_preprocess_u8: the pre-processing alone, pixel_values_dev [1, 3, 512, 512] f32 (two launches, four above 1024).
 */
int nesr_segformer_segment_u8(nesr_segformer* ctx, const uint8_t* rgb_dev, int H, int W, uint8_t* class_map_dev, size_t capacity,
                              int* out_h, int* out_w, void* hip_stream);
int nesr_segformer_preprocess_u8(nesr_segformer* ctx, const uint8_t* rgb_dev, int H, int W, float* pixel_values_dev, void* hip_stream);
/*
 * The launch counter and the event timing of a context.  The counter always runs; with timing on, every launch is bracketed by an
 * event pair and summed into its group.  nesr_segformer_kernel_time_ms waits for the recorded launches, writes the first
 * min(n_groups, NESR_SEG_GROUPS) group times (ms) and the launches since the last call, and resets both.
 */
enum { NESR_SEG_GROUP_PREPROCESS = 0, NESR_SEG_GROUP_PATCH_EMBED = 1, NESR_SEG_GROUP_LN_PROJ = 2, NESR_SEG_GROUP_SEQ_REDUCTION = 3,
       NESR_SEG_GROUP_ATTENTION = 4, NESR_SEG_GROUP_MIX_FFN = 5, NESR_SEG_GROUP_DECODE_HEAD = 6, NESR_SEG_GROUPS = 7 };
int nesr_segformer_set_timing(nesr_segformer* ctx, int enable);
int nesr_segformer_kernel_time_ms(nesr_segformer* ctx, double* group_ms, int n_groups, int64_t* launches);
/*
 * PIL's `Image.resize((out_w, out_h), filter)` of an 8-bit image (nesr/nesr.py:709, and the extractor's resize behind :712) on
 * [H, W, C] u8, C = 1..4, bit for bit: the horizontal pass, then the vertical pass, a u8 image between them, a pass that keeps its
 * size skipped; integer coefficients with 22 fractional bits from doubles computed on the host.  filter: NESR_PIL_LANCZOS (1) or
 * NESR_PIL_BILINEAR (2), PIL.Image's own numbers.  Allocates its tables and the intermediate image and waits for hip_stream
 * on every route (also when the sizes are equal and the image is only copied): dst is written when it returns.
 */
enum { NESR_PIL_LANCZOS = 1, NESR_PIL_BILINEAR = 2 };
int nesr_pil_resize_u8(int device_id, const uint8_t* src_dev, int H, int W, int C, uint8_t* dst_dev, int out_h, int out_w, int filter,
                       void* hip_stream);

/*
 * ---- Swin2SR, a second upscaler for the ensemble (csrc/swin2sr.hip, swin2sr_api.cpp) -- swin2sr.Swin2SR.
 * transformers' Swin2SRForImageSuperResolution in eval mode: f32 storage, every product on the f32-input MFMA.
 *
 * nesr_swin2sr_create takes Swin2SRConfig's fields by name; depths and num_heads hold num_stages (1..16) entries.  The
 * configuration is checked before any device is touched.  NESR_ERR_UNSUPPORTED (the text names the field) for upsampler
 * "pixelshuffle_aux" or any name but pixelshuffle / pixelshuffledirect / nearest+conv, resi_connection other than "1conv",
 * use_absolute_embeddings, patch_size != 1, qkv_bias false, image_size <= window_size, num_heads that differ between stages or do
 * not divide embed_dim, an upscale the head is not built for (pixelshuffle: 2^n or 3; nearest+conv: 4), and a window / width
 * whose working set exceeds the 160 KiB of LDS.  Anything else out of range is NESR_ERR_ARG.
 *
 * nesr_swin2sr_load_weight: keys are transformers' state_dict names (one generation: conversion_mapping.py renames nothing for
 * Swin2SR); an unknown key or a wrong shape is NESR_ERR_ARG; keys ending in relative_position_index, relative_coords_table or
 * attn_mask are accepted and ignored.  nesr_swin2sr_finalize: a missing key is NESR_ERR_STATE; computes each layer's position bias
 * table 16 sigmoid(MLP(table))[index] in double on the host and uploads the padded, transposed weights.
 *
 * nesr_swin2sr_forward_f32: pixel_values_dev [1, C, H, W] f32, H and W multiples of window_size (NESR_ERR_ARG otherwise) ->
 * out_dev [1, num_channels_out, H s, W s] f32; capacity counts floats.  nesr_swin2sr_upscale_u8: an HWC u8 RGB frame of any size ->
 * the HWC u8 frame [H s, W s, 3]; capacity counts bytes.  It does what Swin2SRImageProcessor and the documented post-processing
 * do: / 255, symmetric padding right and bottom to (n / 8 + 1) * 8, the model (with its own reflect padding to the window), the
 * crop, clamp to [0, 1], x 255, round to nearest even; the paddings, the normalisation and the quantiser run inside the first
 * and the last convolution.  A capacity too small is NESR_ERR_ARG before any launch; the workspace grows with the frame
 * (NESR_ERR_NOMEM when it cannot).  nesr_swin2sr_output_size touches no device and needs no context.
 */
typedef struct nesr_swin2sr nesr_swin2sr;
int nesr_swin2sr_create(nesr_swin2sr** out, int device_id, int image_size, int patch_size, int num_channels, int num_channels_out,
                        int embed_dim, int num_stages, const int* depths, const int* num_heads, int window_size, double mlp_ratio,
                        int qkv_bias, int use_absolute_embeddings, double layer_norm_eps, int upscale, double img_range,
                        const char* resi_connection, const char* upsampler);
void nesr_swin2sr_destroy(nesr_swin2sr* ctx);
int nesr_swin2sr_num_tensors(const nesr_swin2sr* ctx);
int nesr_swin2sr_load_weight(nesr_swin2sr* ctx, const char* key, const float* data_host, const int64_t* shape, int ndim);
int nesr_swin2sr_finalize(nesr_swin2sr* ctx);
int nesr_swin2sr_output_size(int upscale, int H, int W, int* out_h, int* out_w);
int nesr_swin2sr_forward_f32(nesr_swin2sr* ctx, const float* pixel_values_dev, int N, int C, int H, int W, float* out_dev, size_t capacity,
                             void* hip_stream);
int nesr_swin2sr_upscale_u8(nesr_swin2sr* ctx, const uint8_t* rgb_dev, int H, int W, uint8_t* out_dev, size_t capacity, void* hip_stream);
/*
 * Tiled frames and batches.  The workspace of the entries above grows with the frame (about 1.3 GB at 512 x 512 for the classical
 * x2 model); a large frame goes through nesr_swin2sr_upscale_tiled_u8 instead, window by window, and equal windows share launches.
 *
 * The plan, per axis of length n with tile = T >= 1 (the core's side, input pixels) and tile_pad = P >= 0: cores i = 0 ..
 * ceil(n / T) - 1, [c0, c1) = [i T, min((i + 1) T, n)); every window of the axis is S = min(T + 2 P, n) long and starts at
 * w0 = clamp(c0 - P, 0, n - S): a window at the edge slides inward instead of shrinking, so all windows of a frame have one shape
 * win_h x win_w, and a core pixel has at least min(P, its distance to the frame's edge) pixels of true context on each side.
 * Each window is treated exactly as a frame given to nesr_swin2sr_upscale_u8; of its output, the core's rows and columns are
 * quantised and stored at the core's place of the H s x W s x 3 result.  A frame with H <= T + 2 P and W <= T + 2 P has one window
 * (the frame) and gives the bits of nesr_swin2sr_upscale_u8.
 *
 * nesr_swin2sr_tile_plan touches no device and needs no context: the counts, the window shape and, unless `plan` is null, one row
 * of 8 integers per tile in row-major order, {win_y, win_x (input pixels), crop_y, crop_x, crop_h, crop_w (the core inside the
 * window's output), out_y, out_x (its place in the result)}, the last six in output pixels; capacity counts integers.
 * nesr_swin2sr_workspace_bytes: what a forward of `batch` windows of win_h x win_w allocates.
 *
 * nesr_swin2sr_upscale_tiled_u8: the tiles run in row-major order in ceil(n / B) batches of B windows, the last one shorter;
 * B = max_batch, or for max_batch <= 0 as many windows as keep the workspace within NESR_SWIN2SR_TILE_WORKSPACE_BYTES (a
 * setting, not a measurement), in both cases at least one and at most the tiles of the frame.  The result does not depend on B.
 * The reflect-padding limit of the model (a window no shorter than half the attention window, roughly) is checked on the
 * window shape before any launch.  NESR_ERR_ARG, before any launch and with the argument's name in the text: tile < 1,
 * tile_pad < 0, a capacity too small, a model whose channels are not 3 / 3.
 *
 * nesr_swin2sr_forward_batch_f32: pixel_values_dev [N, C, H, W] f32, N >= 1 -> out_dev [N, num_channels_out, H s, W s]; every
 * image gets the bits nesr_swin2sr_forward_f32 gives it alone.  H or W no multiple of window_size is NESR_ERR_ARG.
 * Every launch of a batch counts once in nesr_swin2sr_kernel_time_ms.
 */
#define NESR_SWIN2SR_TILE_WORKSPACE_BYTES ((size_t)2 << 30)
#define NESR_SWIN2SR_TILED_MAX_PIXELS (1ll << 28)
int nesr_swin2sr_tile_plan(int upscale, int H, int W, int tile, int tile_pad, int* tiles_y, int* tiles_x, int* win_h, int* win_w, int32_t* plan,
                           size_t capacity);
int nesr_swin2sr_workspace_bytes(nesr_swin2sr* ctx, int win_h, int win_w, int batch, size_t* bytes);
int nesr_swin2sr_upscale_tiled_u8(nesr_swin2sr* ctx, const uint8_t* rgb_dev, int H, int W, int tile, int tile_pad, int max_batch, uint8_t* out_dev,
                                  size_t capacity, void* hip_stream);
int nesr_swin2sr_forward_batch_f32(nesr_swin2sr* ctx, const float* pixel_values_dev, int N, int C, int H, int W, float* out_dev, size_t capacity,
                                   void* hip_stream);
/*
 * Overlapped tiles, averaged: the tiling of the Swin2SR / SwinIR authors' test script (--tile, --tile_overlap).  The frame is / 255
 * and padded ONCE, by its own symmetric extension on the right and bottom, to Hp x Wp, the next multiples of window_size; there is
 * no processor padding to (n / 8 + 1) * 8, of the frame or of a window.  The effective tile is t = min(tile, Hp, Wp).  Per axis of
 * padded length n the tiles start at 0, t - tile_overlap, 2 (t - tile_overlap), ... below n - t, and then at n - t: the last tile
 * slides back to end at the frame's edge and is in general not on the stride.  Every t x t window, in row-major order, goes
 * through the network as it is (t is a multiple of window_size, so the model pads nothing); its f32 output, / img_range + mean and
 * before any clamp, is ADDED into an f32 accumulator of the padded output, in ascending tile index; at the end every pixel is
 * divided by the number of windows that covered it (a true f32 division), cropped to H s x W s, clamped, x 255, rounded to nearest
 * even and stored as HWC u8.  A pixel near a tile's edge is the mean of up to four evaluations (nine when tile_overlap > t / 2).
 *
 * nesr_swin2sr_overlap_plan touches no device and needs no context: tiles_y, tiles_x, t, Hp, Wp and, unless `plan` is null, one row
 * of 4 integers per window in row-major order, {win_y, win_x (input pixels of the padded frame), out_y, out_x (output pixels)};
 * capacity counts integers.  nesr_swin2sr_overlap_workspace_bytes: the network's workspace of `batch` windows, plus their f32
 * outputs, plus the accumulator (12 bytes per padded output pixel).
 *
 * nesr_swin2sr_upscale_overlapped_u8: the windows run in ceil(n / B) batches of B, in order on the stream; B = max_batch, or for
 * max_batch <= 0 as many windows as keep the per-batch part (network workspace and outputs; the accumulator belongs to the frame)
 * within NESR_SWIN2SR_TILE_WORKSPACE_BYTES, at least one and at most the windows of the frame.  The result does not depend on B.
 * Both compute forms take the route (the fp16 form clears and checks its range word once a call: NESR_ERR_RANGE).  NESR_ERR_ARG,
 * before any launch and with the output untouched: tile < 1; an effective tile that is not a multiple of window_size;
 * tile_overlap < 0 or >= the effective tile; a capacity too small; a model whose channels are not 3 / 3.  NESR_ERR_NOMEM when the
 * workspace cannot be allocated.  In nesr_swin2sr_kernel_time_ms the accumulation (one launch a batch) and the division (one a
 * call) count under NESR_S2_GROUP_UPSAMPLE: launches = ceil(n / B) * (launches of one forward + 1) + 1.
 */
int nesr_swin2sr_overlap_plan(int upscale, int window_size, int H, int W, int tile, int tile_overlap, int* tiles_y, int* tiles_x, int* t, int* Hp,
                              int* Wp, int32_t* plan, size_t capacity);
int nesr_swin2sr_overlap_workspace_bytes(nesr_swin2sr* ctx, int H, int W, int tile, int tile_overlap, int batch, size_t* bytes);
int nesr_swin2sr_upscale_overlapped_u8(nesr_swin2sr* ctx, const uint8_t* rgb_dev, int H, int W, int tile, int tile_overlap, int max_batch,
                                       uint8_t* out_dev, size_t capacity, void* hip_stream);
/* The launch counter and the per-group event timing, as nesr_segformer_set_timing / nesr_segformer_kernel_time_ms. */
enum { NESR_S2_GROUP_CONV = 0, NESR_S2_GROUP_PROJ = 1, NESR_S2_GROUP_ATTENTION = 2, NESR_S2_GROUP_MLP = 3, NESR_S2_GROUP_UPSAMPLE = 4,
       NESR_S2_GROUPS = 5 };
int nesr_swin2sr_set_timing(nesr_swin2sr* ctx, int enable);
int nesr_swin2sr_kernel_time_ms(nesr_swin2sr* ctx, double* group_ms, int n_groups, int64_t* launches);
/*
 * The fp16 compute form.  nesr_swin2sr_set_dtype, between nesr_swin2sr_create and nesr_swin2sr_finalize (NESR_ERR_STATE after it):
 * NESR_DTYPE_F32 (the default: the path above, unchanged in launches and in bits) or NESR_DTYPE_F16; NESR_DTYPE_BF16 is
 * NESR_ERR_UNSUPPORTED (eight significand bits cost 0.2 to 0.4 in the logits of cosine attention, whose temperature reaches 100);
 * any other value is NESR_ERR_ARG.  The dtype is checked before the context.
 *
 * NESR_DTYPE_F16: storage in memory stays f32 and so do the activation layout, the workspace and the residual stream.  Every GEMM
 * takes both operands rounded to f16 (nearest even) with f32 products and sums on v_mfma_f32_16x16x32_f16 (a K tail of 16 on
 * v_mfma_f32_16x16x16_f16): the 3x3 convs over token rows, the 1x1 projections, q | k | v, q^ k^T (q^, k^ normalised from the f32
 * q and k with the norm and the quotient in double, then rounded), P V (P the f32 softmax, rounded), output.dense (the context rounded), fc1 and fc2 (the GELU output rounded).
 * Everything else is the f32 arithmetic of the default form, the frame-loading first convolution included.  The summation order
 * inside an MFMA is the hardware's.
 * Range: f16 carries |x| <= 65504.  A weight of one of those GEMMs beyond that (or non-finite) is NESR_ERR_RANGE at
 * nesr_swin2sr_finalize, before any device call.  An activation that is non-finite or beyond +-65504 when it is rounded raises the
 * context's range word; the forward entries (and nesr_swin2sr_part_f32) clear the word in front of their launches, wait for the
 * stream behind them and return NESR_ERR_RANGE then: the output is not valid.  (The f32 form neither waits nor checks.)
 *
 * device_id NESR_SWIN2SR_NO_DEVICE gives nesr_swin2sr_create's context without a device: load_weight, set_dtype and finalize do
 * their host side (the strict loading, the range check, the packing); every entry that would launch is NESR_ERR_STATE.
 *
 * nesr_swin2sr_part_f32 runs ONE launch of the context, in its compute form, on the caller's tokens: in_dev [N][H W][C] f32, dense
 * and of the real width C = embed_dim, -> out_dev of the same shape (capacity counts floats); pitched copies move them into and
 * out of the padded layout.  NESR_S2_PART_ATTENTION: the attention block of layer `layer` of stage `stage` (shifted by half a
 * window when `layer` is odd): tokens + LayerNorm(output.dense(attention)).  NESR_S2_PART_MLP: its MLP block: tokens +
 * LayerNorm(fc2(GELU(fc1(tokens)))).  NESR_S2_PART_STAGE_CONV: the stage's 3x3 convolution, rows to rows (`layer` is ignored).
 * H and W are multiples of window_size.
 */
#define NESR_SWIN2SR_NO_DEVICE (-1)
enum { NESR_S2_PART_ATTENTION = 0, NESR_S2_PART_MLP = 1, NESR_S2_PART_STAGE_CONV = 2 };
int nesr_swin2sr_set_dtype(nesr_swin2sr* ctx, int dtype);
int nesr_swin2sr_part_f32(nesr_swin2sr* ctx, int part, int stage, int layer, const float* in_dev, int N, int H, int W, float* out_dev, size_t capacity,
                          void* hip_stream);

/*
 * ---- The x4 diffusion upscaler's VAE decoder (csrc/vae.hip, vae_api.cpp) -- vae.VaeDecoder.
 *
 * diffusers' AutoencoderKL.decode as StableDiffusionUpscalePipeline calls it: post_quant_conv, conv_in, the mid block (ResnetBlock,
 * single-head attention, ResnetBlock), one UpDecoderBlock2D per entry of block_out_channels in reverse (layers_per_block + 1
 * ResnetBlocks, then nearest x2 + 3x3 conv on every block but the last), GroupNorm, SiLU, conv_out.  f32 throughout: diffusers
 * itself upcasts this VAE.  The output is 2^(num_blocks - 1) times the latent grid.
 *
 * nesr_vae_create takes the configuration's fields by name.  Supported: 2 .. 4 entries of block_out_channels, each a multiple of
 * norm_num_groups and at most 512; layers_per_block 1 .. 4; latent_channels 1 .. 8; out_channels 1 .. 4; act_fn "silu".  Anything
 * else is NESR_ERR_UNSUPPORTED before any device is touched, and the text names the field.  device_id NESR_VAE_NO_DEVICE gives the
 * context without a device: load_weight, finalize and the size queries do their host side, every entry that would launch is
 * NESR_ERR_STATE.
 *
 * nesr_vae_load_weight: keys are diffusers' state_dict names (post_quant_conv.weight, decoder.mid_block.attentions.0.to_q.weight,
 * ...); the attention's legacy names query, key, value, proj_attn are the same tensors.  Strict: an unexpected key or another
 * shape is NESR_ERR_ARG (a caller drops encoder.* and quant_conv.* first); nesr_vae_finalize: a missing key is NESR_ERR_STATE.
 *
 * nesr_vae_decode_f32: z_dev [1, latent_channels, h, w] f32 -> sample_dev [1, out_channels, h s, w s] f32 (capacity counts
 * floats).  nesr_vae_decode_latents_u8 (out_channels 3): latents_dev of the same shape -> the frame [h s, w s, 3] u8 RGB:
 * latents / scaling_factor, decode, / 2 + 0.5, clamp to [0, 1], x 255, round half to even (capacity counts bytes).  N = 1.
 * h w may not exceed NESR_VAE_MAX_TOKENS (the attention's limit) nor h s x w s 2^24 pixels: NESR_ERR_ARG.  The workspace grows
 * with the frame (nesr_vae_workspace_bytes says to what; NESR_ERR_NOMEM when it cannot).  No atomics anywhere: a call repeated
 * gives the same bits.  nesr_vae_output_size touches no device and needs no context.
 *
 * nesr_vae_decode_latents_tiled_u8 lifts the token limit: the decode over overlapping windows of min(tile, h) x min(tile, w)
 * latents, blended on the device by the plan, the weights and the kernels of nesr_sdx4_upscale_tiled_u8 below (per window a
 * gather, the f32 decode with the scaling factor, a blend-add; one finish that normalises and quantises).  h, w, tile and
 * tile_overlap are multiples of 2, 0 <= tile_overlap < the window's sides, a window holds at most NESR_VAE_MAX_TOKENS latents and
 * h w at most 2^22; latents_dev is 8-byte aligned, out_dev 4-byte.  One window gives nesr_vae_decode_latents_u8's bytes.  The
 * context's launch counter and timer see the windows' decodes; the three window kernels (one gather and one blend-add a window,
 * one finish) are the pipeline's, and in this entry they are neither counted nor timed.
 */
#define NESR_VAE_NO_DEVICE (-1)
#define NESR_VAE_MAX_TOKENS (1 << 16)
typedef struct nesr_vae nesr_vae;
int nesr_vae_create(nesr_vae** out, int device_id, int latent_channels, int out_channels, int num_blocks, const int* block_out_channels,
                    int layers_per_block, int norm_num_groups, double scaling_factor, const char* act_fn);
void nesr_vae_destroy(nesr_vae* ctx);
int nesr_vae_num_tensors(const nesr_vae* ctx);
int nesr_vae_load_weight(nesr_vae* ctx, const char* key, const float* data_host, const int64_t* shape, int ndim);
int nesr_vae_finalize(nesr_vae* ctx);
int nesr_vae_output_size(int num_blocks, int h, int w, int* out_h, int* out_w);
int nesr_vae_workspace_bytes(nesr_vae* ctx, int h, int w, size_t* bytes);
int nesr_vae_decode_f32(nesr_vae* ctx, const float* z_dev, int N, int C, int h, int w, float* sample_dev, size_t capacity, void* hip_stream);
int nesr_vae_decode_latents_u8(nesr_vae* ctx, const float* latents_dev, int N, int C, int h, int w, uint8_t* out_dev, size_t capacity,
                               void* hip_stream);
int nesr_vae_decode_latents_tiled_u8(nesr_vae* ctx, const float* latents_dev, int N, int C, int h, int w, int tile, int tile_overlap, uint8_t* out_dev,
                                     size_t capacity, void* hip_stream);
/* Kernel groups of nesr_vae_kernel_time_ms, as nesr_swin2sr_kernel_time_ms: the 3x3 convs, the GroupNorm statistics, the streamed
 * attention, the 1x1 products (post_quant_conv, shortcuts, q | k | v, to_out, and the latents' transposition), the nearest-x2 convs. */
enum { NESR_VAE_GROUP_CONV = 0, NESR_VAE_GROUP_NORM = 1, NESR_VAE_GROUP_ATTENTION = 2, NESR_VAE_GROUP_PROJ = 3, NESR_VAE_GROUP_UPSAMPLE = 4,
       NESR_VAE_GROUPS = 5 };
int nesr_vae_set_timing(nesr_vae* ctx, int enable);
int nesr_vae_kernel_time_ms(nesr_vae* ctx, double* group_ms, int n_groups, int64_t* launches);

/*
 * ---- The x4 diffusion upscaler's UNet (csrc/unet.hip, unet_api.cpp) -- unet.UNet2DCondition.
 *
 * diffusers' UNet2DConditionModel.forward as StableDiffusionUpscalePipeline calls it: the timestep's sinusoid through
 * time_embedding plus the class row (the pipeline's noise level), conv_in, the down blocks (ResnetBlocks, each followed by a
 * Transformer in a CrossAttnDownBlock2D, then a stride-2 conv), the mid block, the up blocks over cat(hidden, skip) (then nearest
 * x2 + conv), GroupNorm, SiLU, conv_out.  f32 throughout.  The output has the input's grid.
 *
 * nesr_unet_create takes the configuration's fields by name; attention_head_dim is, as in this model family, the NUMBER of heads
 * of every block.  Supported: 2 .. 4 levels; block types DownBlock2D, CrossAttnDownBlock2D, UpBlock2D, CrossAttnUpBlock2D and the
 * mid block UNetMidBlock2DCrossAttn; layers_per_block 1 .. 3; widths up to 1024 that are multiples of norm_num_groups and, where
 * the level has attention, of the heads, with a head width of 8 .. 128 that is a multiple of 8; cross_attention_dim up to 1024;
 * in_channels and out_channels up to 16; use_linear_projection true; one transformer layer; no dual_cross_attention; act_fn "silu";
 * flip_sin_to_cos true, freq_shift 0, downsample_padding 1; a class embedding table.  Anything else is NESR_ERR_UNSUPPORTED before
 * any device is touched, and the text names the field.  only_cross_attention has one flag a level (down block order); up block i
 * takes the flag and the width of level num_blocks - 1 - i.  device_id NESR_UNET_NO_DEVICE gives the context without a device.
 *
 * nesr_unet_load_weight: keys are diffusers' state_dict names (time_embedding.linear_1.weight, down_blocks.1.attentions.0.
 * transformer_blocks.0.attn1.to_q.weight, ...).  Strict, as nesr_vae_load_weight.
 *
 * nesr_unet_forward_f32: sample_dev [n, in_channels, h, w] f32, text_states_dev [n, tokens, cross_attention_dim] f32 ->
 * out_dev [n, out_channels, h, w] f32; out_elems must be exactly that count.  n is 1 or 2: the samples share the timestep and
 * the class label and carry their own text states (classifier-free guidance).  h and w are multiples of 2^(num_blocks - 1),
 * tokens is 1 .. NESR_UNET_MAX_TEXT_TOKENS, class_label indexes the table, a self-attention takes at most 65536 tokens: otherwise
 * NESR_ERR_ARG before any launch.  The workspace holds the skip stack and grows with the frame (NESR_ERR_NOMEM when it cannot).
 * No atomics anywhere: a call repeated gives the same bits, and a sample's result does not depend on n.
 */
#define NESR_UNET_NO_DEVICE (-1)
#define NESR_UNET_MAX_TEXT_TOKENS 256
typedef struct nesr_unet nesr_unet;
int nesr_unet_create(nesr_unet** out, int device_id, int in_channels, int out_channels, int num_blocks, const int* block_out_channels,
                     const char* const* down_block_types, const char* const* up_block_types, const char* mid_block_type,
                     const int* only_cross_attention, int layers_per_block, int attention_head_dim, int cross_attention_dim,
                     int transformer_layers_per_block, int use_linear_projection, int dual_cross_attention, int num_class_embeds,
                     int norm_num_groups, double norm_eps, int flip_sin_to_cos, double freq_shift, int downsample_padding, const char* act_fn);
void nesr_unet_destroy(nesr_unet* ctx);
int nesr_unet_num_tensors(const nesr_unet* ctx);
int nesr_unet_load_weight(nesr_unet* ctx, const char* key, const float* data_host, const int64_t* shape, int ndim);
int nesr_unet_finalize(nesr_unet* ctx);
int nesr_unet_workspace_bytes(nesr_unet* ctx, int n, int h, int w, int tokens, size_t* bytes);
int nesr_unet_forward_f32(nesr_unet* ctx, const float* sample_dev, int n, int c, int h, int w, double timestep, int class_label,
                          const float* text_states_dev, int tokens, float* out_dev, size_t out_elems, void* hip_stream);
/* Kernel groups of nesr_unet_kernel_time_ms: the 3x3 convs, the GroupNorm and LayerNorm statistics, the streamed attention, the
 * projections (proj_in / proj_out, q, k | v, to_out, shortcuts, the inputs' transposition), the feed-forward's two products, the
 * embedding path, the stride-2 and nearest-x2 convs. */
enum { NESR_UNET_GROUP_CONV = 0, NESR_UNET_GROUP_NORM = 1, NESR_UNET_GROUP_ATTENTION = 2, NESR_UNET_GROUP_PROJ = 3, NESR_UNET_GROUP_FF = 4,
       NESR_UNET_GROUP_EMBEDDING = 5, NESR_UNET_GROUP_RESAMPLE = 6, NESR_UNET_GROUPS = 7 };
int nesr_unet_set_timing(nesr_unet* ctx, int enable);
int nesr_unet_kernel_time_ms(nesr_unet* ctx, double* group_ms, int n_groups, int64_t* launches);
/*
 * The fp16 compute form.  nesr_unet_set_dtype, between nesr_unet_create and nesr_unet_finalize (NESR_ERR_STATE after it):
 * NESR_DTYPE_F32 (the default: the path above, unchanged in launches and in bits) or NESR_DTYPE_F16; NESR_DTYPE_BF16 and every
 * other value are NESR_ERR_UNSUPPORTED, and the text names the value.  The dtype is checked before the context.  nesr_unet_dtype
 * reads it back.
 *
 * NESR_DTYPE_F16: storage in memory stays f32 in and out, and so do the layouts, the workspace, the skip stack and the residual
 * stream; a forward makes the same number of launches, each f16 launch in the place of one f32 launch.  Both operands of every
 * 3x3 conv (conv_in, the ResnetBlocks' convs, the downsamplers, the up-convs, conv_out) and of every row product (the 1x1
 * shortcuts, proj_in / proj_out, q, q | k | v, the text's k | v, to_out, ff.net.0.proj, ff.net.2) are rounded to f16 (nearest
 * even, a plain cast) with f32 products and sums on v_mfma_f32_16x16x32_f16 (a K tail of 16 on v_mfma_f32_16x16x16_f16).  The
 * activation is rounded AFTER its prologue (GroupNorm + SiLU, GroupNorm, LayerNorm, each evaluated in f32); a padding tap is 0.
 * Biases, residuals, GEGLU's (h + b_h) gelu(g + b_g), the norms' statistics, the streamed attention on the f32 q, k, v, the
 * embedding and time_emb_proj stay the f32 form's arithmetic.  An operand that rounds to an f16 subnormal (below 6.1e-5 in
 * magnitude) is KEPT by the MI355X's matrix cores, not flushed to zero.  An output element's K chain runs in one workgroup in
 * ascending k, so a call repeated gives the same bits and a sample's result does not depend on n, as in the f32 form.
 * The device then holds the f16 copy of those weights and NOT their f32 form: nesr_unet_weight_bytes gives what finalize uploads.
 *
 * Range: f16 carries |x| <= 65504.  A weight of one of those products beyond that (or non-finite) is NESR_ERR_RANGE at
 * nesr_unet_finalize, before any device call, and the text names the key (a context of NESR_UNET_NO_DEVICE reaches this on the
 * CPU); the embedding's and time_emb_proj's weights are not rounded and not checked.  An activation that is non-finite or beyond
 * +-65504 when it is rounded raises the context's range word; nesr_unet_forward_f32 on such a context clears the word in front
 * of its launches, waits for the stream behind them and returns NESR_ERR_RANGE then: the output is not valid.  So an fp16 forward
 * is synchronous; the f32 form neither waits nor checks.
 *
 * nesr_unet_pack_linear_f16 / nesr_unet_pack_conv_f16: the packing finalize applies to one such weight, on the host, stateless.
 * weight [n][k0 + k1] (torch's Linear, or a 1x1 conv over a concatenation of k0 | k1 channels; k1 = 0: one source) ->
 * out [round16(n)][round16(k0) + round16(k1)] f16, k contiguous, source 1's k from round16(k0), zeros elsewhere; weight
 * [n][c0 + c1][3][3] -> out [round16(n)][9 taps][round16(c0) + round16(c1)].  out_halves must be exactly that count.
 * NESR_ERR_RANGE for a value f16 cannot carry.
 */
int nesr_unet_set_dtype(nesr_unet* ctx, int dtype);
int nesr_unet_dtype(const nesr_unet* ctx);
int nesr_unet_weight_bytes(const nesr_unet* ctx, size_t* bytes);
int nesr_unet_pack_linear_f16(const float* weight_host, int n, int k0, int k1, uint16_t* out_host, size_t out_halves);
int nesr_unet_pack_conv_f16(const float* weight_host, int n, int c0, int c1, uint16_t* out_host, size_t out_halves);

/*
 * Single-launch entries of the UNet's kernels (test hooks for the per-launch parity tests, csrc/unet_kernel_api.cpp; not pipeline
 * entries): each fills one launcher's arguments, field for field as csrc/unet_api.h documents them, and makes that one launch on
 * hip_stream.  Asynchronous; no context, nothing allocated, no state changed.  Every pointer is a DEVICE pointer in the kernels'
 * own layout, which the caller packs: activations are rows [n m][cs], cs = the width rounded up to 16 and the columns past the
 * width zero; a weight matrix is Wt[K][N], a conv's [9 (cinp0 + cinp1)][coutp] with each source's K rounded up to 4; a norm is
 * [n][cs] x (mean hi, mean lo, gamma rstd, beta) f32; LayerNorm statistics are [m] x (mean hi, mean lo, rstd, 0) f32.  A second
 * source is absent when in1_dev is null.  What a launcher refuses is NESR_ERR_ARG with nothing launched (nesr_last_error names
 * the launcher); the extents are not checked against the buffers, which are the caller's.
 *   nesr_unet_k_in                NCHW [n][c][m] (rows = n m) or row-major [rows][c] -> rows [rows][cs]
 *   nesr_unet_k_embedding         silu(linear_2(silu(linear_1([cos | sin](t)))) + the class row) -> out [tdp]
 *   nesr_unet_k_temb              out[r][0 .. coutp[r]) of [count][1024] = weights[cb + c] + weights[b + c] + sum_k semb[k] weights[w + k coutp + c]
 *                                 (the offset and coutp arrays are HOST arrays of `count` entries, offsets in floats)
 *   nesr_unet_k_conv              3x3 / pad 1 over one or two sources, GroupNorm + SiLU in the loader where a norm is given; stride 1
 *                                 (up: over the nearest-x2 grid of (H / 2) x (W / 2) rows) or stride 2 (the input grid is 2H x 2W);
 *                                 H x W is the OUTPUT grid; + res; rows [n H W][coutp] or NCHW [n][cout][H][W]
 *   nesr_unet_k_group_norm        the statistics of one or two sources side by side in `groups` groups (a partial launch per source, then
 *                                 the finish): norm0_dev / norm1_dev are the OUTPUT, partial*_dev [n][ceil(m / 512)][cs][2] f64 scratch
 *   nesr_unet_k_layer_norm_stats  per row of [m][cs] the mean and 1 / sqrt(var + eps) over the c real columns
 *   nesr_unet_k_rows              rows -> prologue (0 none | 1 GroupNorm | 2 LayerNorm) -> x Wt + b -> (+ res | GEGLU) -> out [m][np]
 *   nesr_unet_k_attention         softmax(q k^T / sqrt(d)) v per sample and head; out [samples nq][ldo], its columns past heads d zeroed
 */
int nesr_unet_k_in(const float* src_dev, int nchw, int c, int cs, int m, long long rows, float* out_dev, void* hip_stream);
int nesr_unet_k_embedding(double timestep, int c0, int td, int tdp, const float* w1_dev, const float* b1_dev, const float* w2_dev, const float* b2_dev,
                          const float* cls_dev, float* out_dev, void* hip_stream);
int nesr_unet_k_temb(int count, int td, const float* semb_dev, const float* weights_dev, const unsigned long long* w_offset,
                     const unsigned long long* b_offset, const unsigned long long* cb_offset, const int* coutp, float* out_dev, void* hip_stream);
int nesr_unet_k_conv(int n, int H, int W, int stride, int up, const float* in0_dev, int c0, int cs0, const void* norm0_dev, const float* in1_dev, int c1,
                     int cs1, const void* norm1_dev, const float* w_dev, const float* bias_dev, int cout, int coutp, const float* res_dev, int out_nchw,
                     float* out_dev, void* hip_stream);
int nesr_unet_k_group_norm(int n, int m, const float* in0_dev, int c0, int cs0, void* norm0_dev, double* partial0_dev, const float* in1_dev, int c1, int cs1,
                           void* norm1_dev, double* partial1_dev, int groups, const float* gamma_dev, const float* beta_dev, float eps, void* hip_stream);
int nesr_unet_k_layer_norm_stats(const float* in_dev, int m, int c, int cs, float eps, void* out_dev, void* hip_stream);
int nesr_unet_k_rows(int m, int rows_per_sample, const float* in0_dev, int c0, int cs0, const void* norm0_dev, const float* in1_dev, int c1, int cs1,
                     const void* norm1_dev, int prologue, const void* ln_dev, const float* ln_g_dev, const float* ln_b_dev, const float* w_dev,
                     const float* b_dev, int ldw, int np, int geglu, const float* res_dev, float* out_dev, void* hip_stream);
int nesr_unet_k_attention(int samples, int nq, int nk, int heads, int d, const float* q_dev, const float* k_dev, const float* v_dev, int ldq, int ldkv,
                          int ldo, float* out_dev, void* hip_stream);
/*
 * The fp16 form's two launches (csrc/unet_f16_kernel_api.cpp): the arguments of nesr_unet_k_conv / nesr_unet_k_rows, with the
 * weight as the DEVICE pointer w16_dev to its f16 packing, 16-byte aligned: rows W16[ldw][cs0 + cs1], conv
 * W16[coutp][9][cs0 + cs1] (each source's K is its row width cs, not the width rounded up to 4), k contiguous.  range_dev: a
 * DEVICE word the launch raises (stores 1) when an activation is non-finite or beyond +-65504 as it is rounded, or null.
 * block_host: where the output columns (conv: channels) of a workgroup that the launcher picked from the shape, 128, 64 or 32,
 * are written on the host, or null.
 */
int nesr_unet_k_conv_f16(int n, int H, int W, int stride, int up, const float* in0_dev, int c0, int cs0, const void* norm0_dev, const float* in1_dev,
                         int c1, int cs1, const void* norm1_dev, const void* w16_dev, const float* bias_dev, int cout, int coutp, const float* res_dev,
                         int out_nchw, float* out_dev, unsigned* range_dev, int* block_host, void* hip_stream);
int nesr_unet_k_rows_f16(int m, int rows_per_sample, const float* in0_dev, int c0, int cs0, const void* norm0_dev, const float* in1_dev, int c1, int cs1,
                         const void* norm1_dev, int prologue, const void* ln_dev, const float* ln_g_dev, const float* ln_b_dev, const void* w16_dev,
                         const float* b_dev, int ldw, int np, int geglu, const float* res_dev, float* out_dev, unsigned* range_dev, int* block_host,
                         void* hip_stream);

/*
 * Single-launch entries of the VAE decoder's kernels (test hooks as the nesr_unet_k_* above, csrc/vae_kernel_api.cpp): each fills
 * one launcher's arguments, field for field as csrc/vae_api.h documents them, and makes that one launch on hip_stream.
 * Asynchronous; no context, nothing allocated, no state changed.  Every pointer is a DEVICE pointer in the kernels' own layout:
 * rows [H W][cs], a 3x3 weight [9 cinp][coutp] with cinp the input width rounded up to 4, a 1x1 weight [cs_in][np], a norm
 * [cs] x (mean hi, mean lo, gamma rstd, beta) f32.  What a launcher refuses is NESR_ERR_ARG with nothing launched
 * (nesr_last_error names the launcher); the extents are not checked against the buffers, which are the caller's.
 *   nesr_vae_k_in          z NCHW [c][m] -> rows [m][16], each value divided by `divisor`; the columns past c zero
 *   nesr_vae_k_conv        3x3 / pad 1 on the H x W grid; in_mode 0 rows | 1 the nearest-x2 grid of (H / 2) x (W / 2) rows; GroupNorm +
 *                          SiLU in the loader where a norm is given; + bias + res[.][cs_res]; out_mode 0 rows [H W][cs_out = coutp] |
 *                          1 NCHW f32 [cout][H][W] | 2 HWC u8 [H][W][cout] (v / 2 + 0.5, clamp, x 255, round to nearest even)
 *   nesr_vae_k_group_norm  the statistics of rows [m][cs] in `groups` groups (the partial launch, then the finish): norm_dev [cs] is the
 *                          OUTPUT, partial_dev [ceil(m / 512)][cs][2] f64 scratch
 *   nesr_vae_k_rows        rows [m][cs_in] -> (norm, no activation) -> x Wt + b -> + res -> out [m][np]; out may be in when np == cs_in
 *   nesr_vae_k_attention   qkv [n][3 cs] (q | k | v) -> out [n][cs] = softmax(q k^T / sqrt(c)) v, one head
 */
int nesr_vae_k_in(const float* z_dev, int c, int m, float divisor, float* out_dev, void* hip_stream);
int nesr_vae_k_conv(int in_mode, const float* in_dev, int H, int W, int cin, int cinp, int cs_in, const void* norm_dev, const float* w_dev,
                    const float* bias_dev, int cout, int coutp, const float* res_dev, int cs_res, int out_mode, void* out_dev, int cs_out,
                    void* hip_stream);
int nesr_vae_k_group_norm(const float* in_dev, int m, int c, int cs, int groups, double* partial_dev, const float* gamma_dev, const float* beta_dev,
                          float eps, void* norm_dev, void* hip_stream);
int nesr_vae_k_rows(int m, int cs_in, int np, const float* in_dev, const void* norm_dev, const float* w_dev, const float* b_dev, const float* res_dev,
                    float* out_dev, void* hip_stream);
int nesr_vae_k_attention(int n, int c, int cs, const float* qkv_dev, float* out_dev, void* hip_stream);

/*
 * ---- The x4 diffusion upscaler's text encoder (csrc/clip_text.hip, clip_text_api.cpp) -- clip_text.ClipTextEncoder.
 *
 * transformers' CLIPTextModel(input_ids)[0] in eval mode, f32: token row + position row (positions from 0), then per layer
 * x += out_proj(attn(layer_norm1(x))) and x += fc2(act(fc1(layer_norm2(x)))), then final_layer_norm on every position.  The
 * attention is causal (query i sees keys 0 .. i), its heads are contiguous column blocks of q, k and v, its scores are scaled by
 * 1 / sqrt(head width).  No attention mask is taken, as the x4 pipeline passes none: a padding id is an ordinary token.  The
 * pooled output and text_projection are not computed.
 *
 * nesr_clip_text_create takes the configuration's fields by name.  Supported: hidden_size up to 1024 that is a multiple of
 * num_attention_heads with a head width of 8 .. 128 that is a multiple of 8; intermediate_size up to 4096; any positive layer
 * count, vocabulary and max_position_embeddings; hidden_act "gelu" (erf) or "quick_gelu" (x sigmoid(1.702 x)).  Anything else is
 * NESR_ERR_UNSUPPORTED before any device is touched, and the text names the field.  device_id NESR_CLIP_TEXT_NO_DEVICE gives the
 * context without a device (the host side alone: strict loading and packing; every entry that would launch is NESR_ERR_STATE).
 *
 * nesr_clip_text_load_weight: keys are transformers' state_dict names of either generation: embeddings.token_embedding.weight,
 * encoder.layers.0.self_attn.k_proj.weight, ..., final_layer_norm.bias, or the same behind "text_model." as published
 * text_encoder/ files carry them; their embeddings.position_ids buffer is accepted and ignored.  Strict, as nesr_vae_load_weight;
 * nesr_clip_text_finalize: a missing key is NESR_ERR_STATE.
 *
 * nesr_clip_text_encode_f32: ids_host [n, tokens] int32 on the HOST (a tokenizer's output; read before the entry returns) ->
 * out_dev [n, tokens, hidden_size] f32, which is what nesr_unet_forward_f32 takes as text_states_dev; out_elems must be exactly
 * that count.  n is 1 or 2, tokens 1 .. min(max_position_embeddings, NESR_UNET_MAX_TEXT_TOKENS), every id indexes the table:
 * otherwise NESR_ERR_ARG before any launch.  Asynchronous on hip_stream: the ids travel in a launch's arguments, nothing is copied
 * or synchronised once the workspace has its size (nesr_clip_text_workspace_bytes; it grows with n tokens).  3 + 8 layers
 * launches, whatever n and tokens.  No atomics anywhere: a call repeated gives the same bits, and a sample's result does not
 * depend on n.
 */
#define NESR_CLIP_TEXT_NO_DEVICE (-1)
typedef struct nesr_clip_text nesr_clip_text;
int nesr_clip_text_create(nesr_clip_text** out, int device_id, int vocab_size, int hidden_size, int intermediate_size, int num_hidden_layers,
                          int num_attention_heads, int max_position_embeddings, double layer_norm_eps, const char* hidden_act);
void nesr_clip_text_destroy(nesr_clip_text* ctx);
int nesr_clip_text_num_tensors(const nesr_clip_text* ctx);
int nesr_clip_text_load_weight(nesr_clip_text* ctx, const char* key, const float* data_host, const int64_t* shape, int ndim);
int nesr_clip_text_finalize(nesr_clip_text* ctx);
int nesr_clip_text_workspace_bytes(nesr_clip_text* ctx, int n, int tokens, size_t* bytes);
int nesr_clip_text_encode_f32(nesr_clip_text* ctx, const int32_t* ids_host, int n, int tokens, float* out_dev, size_t out_elems, void* hip_stream);
/* Kernel groups of nesr_clip_text_kernel_time_ms: the embedding gather, the LayerNorm statistics and the final LayerNorm, the
 * q | k | v and out_proj products, the causal attention, fc1 with its activation and fc2. */
enum { NESR_CLIP_TEXT_GROUP_EMBEDDING = 0, NESR_CLIP_TEXT_GROUP_NORM = 1, NESR_CLIP_TEXT_GROUP_PROJ = 2, NESR_CLIP_TEXT_GROUP_ATTENTION = 3,
       NESR_CLIP_TEXT_GROUP_FF = 4, NESR_CLIP_TEXT_GROUPS = 5 };
int nesr_clip_text_set_timing(nesr_clip_text* ctx, int enable);
int nesr_clip_text_kernel_time_ms(nesr_clip_text* ctx, double* group_ms, int n_groups, int64_t* launches);
/*
 * Single-launch entries of the text encoder's own kernels (test hooks as the nesr_unet_k_* above; csrc/clip_text_api.h documents
 * the launchers' arguments).  Device pointers in the kernels' own layout; what a launcher refuses is NESR_ERR_ARG with nothing launched.
 *   nesr_clip_text_k_embed      out [rows][cs] = tok [vocab][c] at ids_host[row] (a HOST array of `rows` ids) + pos [positions][c] at
 *                               row % tokens, zero past c; an id outside the table or tokens above `positions` is refused
 *   nesr_clip_text_k_attention  causal softmax(q k^T / sqrt(d)) v per sample and head: q, k, v [samples tokens][ld], out [samples
 *                               tokens][ldo], its columns past heads d zeroed
 */
int nesr_clip_text_k_embed(const int32_t* ids_host, int rows, int tokens, const float* tok_dev, int vocab, const float* pos_dev, int positions, int c, int cs,
                           float* out_dev, void* hip_stream);
int nesr_clip_text_k_attention(int samples, int tokens, int heads, int d, const float* q_dev, const float* k_dev, const float* v_dev, int ldq, int ldkv, int ldo,
                               float* out_dev, void* hip_stream);

/*
 * ---- The x4 diffusion upscaler as one call (csrc/sdx4_step.hip, sdx4_api.cpp) -- sdx4.StableDiffusionX4Upscaler.
 *
 * StableDiffusionUpscalePipeline's loop (nesr/nesr.py:988-1031 calls it): the prompts through the text encoder; the u8 frame as
 * v / 127.5 - 1 with the low-res scheduler's add_noise at noise_level; `steps` times the UNet on cat(latents, noised image) with
 * the noise level as class label, classifier-free guidance m = m_neg + g (m_prompt - m_neg), the DDIM step (eta 0); the VAE decoder
 * and its quantiser.  The schedulers' values are recalled from diffusers, not checked against the library or a file (DESIGN
 * section 20 lists each).  Their tables are computed on the host in double; a step reaches the device as six f32 coefficients.
 *
 * nesr_sdx4_create takes the three contexts (not owned: they outlive the pipeline, and nesr_sdx4_destroy leaves them) and the
 * scheduler fields by name.  DDIM: beta_schedule "scaled_linear" (linspace(sqrt(beta_start), sqrt(beta_end), T)^2) or "linear",
 * prediction_type "v_prediction" or "epsilon", clip_sample false, timestep_spacing "leading", steps_offset 0 or 1, eta 0; the
 * final alpha-bar is alpha-bar[0] unless set_alpha_to_one.  Low-res: "squaredcos_cap_v2".  Anything else is NESR_ERR_UNSUPPORTED
 * naming the field.  The contexts must fit each other, else NESR_ERR_ARG naming the mismatch: the UNet's in_channels = the VAE's
 * latent_channels + 3 and its out_channels = latent_channels, cross_attention_dim = the text encoder's hidden_size, a class table
 * larger than max_noise_level, a VAE of 3 out_channels, all three on one device.
 *
 * nesr_sdx4_upscale_u8: frame_dev [h, w, 3] u8 RGB -> out_dev [h s, w s, 3] u8 RGB, s = the VAE's scale (4); capacity counts
 * bytes.  ids_host [n, tokens] int32 on the HOST, n = 2 in the order [negative, prompt] when guidance_scale > 1, else n = 1 (the
 * prompt; no combination).  noise_dev [3, h, w] and latents_dev [latent_channels, h, w] f32 are the caller's unit normal draws
 * (16-byte aligned; a C host brings its own generator).  latents_out_dev, if not null, receives the final f32 latents (one
 * device-to-device copy queued after the last launch).  Every launch goes on hip_stream; once the workspaces have their size
 * (nesr_sdx4_workspace_bytes is the pipeline's own: the text states, the UNet's input and output, the latents) there is no
 * synchronisation, no copy to or from the host and no allocation between the first launch and the last.  h and w must be
 * multiples of 2^(UNet levels - 1) and h w at most NESR_VAE_MAX_TOKENS; tokens, the ids, noise_level (0 .. max_noise_level) and
 * steps (the first timestep must lie in the table) are checked too: NESR_ERR_ARG before any launch.
 *
 * nesr_sdx4_launches: the kernel launches of the last nesr_sdx4_upscale_u8: text + 1 + steps (UNet + 1) + VAE.
 * nesr_sdx4_set_timing / nesr_sdx4_kernel_time_ms time the pipeline's own kernels (the networks have their own timers): the two of
 * the untiled call and, in groups 2 .. 6, the five of the tiled one.
 *
 * nesr_sdx4_schedule and nesr_sdx4_noise_coefficients need no context and no device: the tables a pipeline of these fields
 * uses.  timesteps [steps], alpha_bars [steps][2] (at the step, at the previous step), coefficients [steps][6] (c0x, c0m, cex,
 * cem, sp, sq: x0 = c0x x + c0m m, e = cex x + cem m, x' = sp x0 + sq e); noise coefficients (sqrt(abar_L), sqrt(1 - abar_L)).
 * Null outputs are skipped.
 */
typedef struct nesr_sdx4 nesr_sdx4;
int nesr_sdx4_create(nesr_sdx4** out, nesr_clip_text* text, nesr_unet* unet, nesr_vae* vae, int num_train_timesteps, double beta_start, double beta_end,
                     const char* beta_schedule, const char* prediction_type, int clip_sample, int set_alpha_to_one, int steps_offset,
                     const char* timestep_spacing, double eta, int low_res_num_train_timesteps, const char* low_res_beta_schedule, int max_noise_level);
void nesr_sdx4_destroy(nesr_sdx4* p);
int nesr_sdx4_workspace_bytes(nesr_sdx4* p, int n, int h, int w, int tokens, size_t* bytes);
int nesr_sdx4_upscale_u8(nesr_sdx4* p, const uint8_t* frame_dev, int h, int w, const int32_t* ids_host, int tokens, const float* noise_dev,
                         const float* latents_dev, int noise_level, int steps, double guidance_scale, uint8_t* out_dev, size_t capacity,
                         float* latents_out_dev, void* hip_stream);
int nesr_sdx4_launches(const nesr_sdx4* p, int64_t* launches);
/*
 * Frames above NESR_VAE_MAX_TOKENS low-res pixels: the denoising loop and the VAE decode over overlapping windows of one shape
 * (csrc/sdx4_tiled.hip).  The specification is this project's own (MultiDiffusion-style: one shared latent
 * frame); how diffusers tiles is recalled, not checked, and its enable_vae_tiling blend is not reproduced.
 *
 * The plan, per axis of the low-res frame (sides that are multiples of `multiple` = 2^(UNet levels - 1), which must be even): a
 * window is t = min(tile, n) long; the windows start at 0, t - overlap, ... below n - t, then at n - t (the last one ends at the
 * edge and is in general not on the stride).  tile and tile_overlap are multiples of `multiple`, 0 <= tile_overlap < t on both
 * axes, and a window holds at most NESR_VAE_MAX_TOKENS pixels.  Windows run in row-major order and all have the shape ty x tx.  A
 * window [a, a + t) weighs pixel i of its axis by min(left, right), left = (a > 0 && R > 0) ? min(i - a + 1, R) / R : 1, right =
 * (a + t < n && R > 0) ? min(a + t - i, R) / R : 1, R = tile_overlap: the sides on the frame's edge are not ramped.  w(y, x) =
 * w_y(y) w_x(x); a pixel's normaliser is S(y, x) = Sy(y) Sx(x), each the sum of the axis weights of the windows that cover it, in
 * ascending order.  At the output resolution the same rule holds with origin, length and ramp times the VAE's scale.
 *
 * nesr_sdx4_tile_plan needs no device and no context: tiles_y, tiles_x, ty, tx and, unless `plan` is null, one row (y, x) per
 * window in row-major order (capacity counts integers).  nesr_sdx4_tiled_workspace_bytes needs neither: the pipeline's own bytes
 * of a tiled call (text states, the full-frame buffer [lc + 3][h w], the accumulator [lc][h w], one window's UNet input and
 * output, one VAE window's latents and f32 sample, the f32 frame [h s][w s][3]); the networks report their own for the window.
 *
 * nesr_sdx4_upscale_tiled_u8: the arguments of nesr_sdx4_upscale_u8 and the two plans; vae_tile 0 stands for tile, vae_overlap
 * below 0 for tile_overlap.  noise_dev and latents_dev are full-frame draws.  Per step and window: a gather of the window's
 * UNet input, the UNet forward, an accumulate of w times the guided output; per step one kernel divides by S and takes the DDIM
 * step.  Then per VAE window: a gather, the f32 decode, a blend-add; one finish kernel divides by S and quantises.  Windows run
 * one after the other on hip_stream, so there are no atomics and a repeated call gives the same bits; with one window the call
 * returns nesr_sdx4_upscale_u8's bits.  Checked before any launch (NESR_ERR_ARG naming the value): the multiples, the overlap's
 * range, the window's token limit, capacity, alignment (noise and latents 16 bytes, frame and output 4), h w at most 2^22.  Once
 * the workspaces have their size there is no synchronisation, host copy or allocation between the first launch and the last; an
 * fp16 UNet's range word is cleared once in front and read once behind, as in nesr_sdx4_upscale_u8.
 * nesr_sdx4_launches after it: text + 1 + steps (windows (1 + UNet + 1) + 1) + vae_windows (1 + VAE + 1) + 1.
 */
int nesr_sdx4_tile_plan(int h, int w, int multiple, int tile, int tile_overlap, int* tiles_y, int* tiles_x, int* ty, int* tx, int32_t* plan, size_t capacity);
int nesr_sdx4_tiled_workspace_bytes(int n, int latent_channels, int text_hidden, int vae_scale, int h, int w, int tokens, int multiple, int tile, int tile_overlap,
                                    int vae_tile, int vae_overlap, size_t* bytes);
int nesr_sdx4_upscale_tiled_u8(nesr_sdx4* p, const uint8_t* frame_dev, int h, int w, const int32_t* ids_host, int tokens, const float* noise_dev,
                               const float* latents_dev, int noise_level, int steps, double guidance_scale, int tile, int tile_overlap, int vae_tile,
                               int vae_overlap, uint8_t* out_dev, size_t capacity, float* latents_out_dev, void* hip_stream);
enum { NESR_SDX4_GROUP_PREPARE = 0, NESR_SDX4_GROUP_STEP = 1, NESR_SDX4_GROUP_GATHER = 2, NESR_SDX4_GROUP_ACCUMULATE = 3, NESR_SDX4_GROUP_TILED_STEP = 4,
       NESR_SDX4_GROUP_BLEND_ADD = 5, NESR_SDX4_GROUP_BLEND_FINISH = 6, NESR_SDX4_GROUPS = 7 };
int nesr_sdx4_set_timing(nesr_sdx4* p, int enable);
int nesr_sdx4_kernel_time_ms(nesr_sdx4* p, double* group_ms, int n_groups, int64_t* launches);
int nesr_sdx4_schedule(int num_train_timesteps, double beta_start, double beta_end, const char* beta_schedule, const char* prediction_type,
                       int set_alpha_to_one, int steps_offset, const char* timestep_spacing, int steps, int* timesteps, double* alpha_bars,
                       float* coefficients);
int nesr_sdx4_noise_coefficients(int num_train_timesteps, const char* beta_schedule, int noise_level, double* alpha_bar, float* coefficients);
/*
 * Single-launch entries of the pipeline's two kernels (test hooks as the nesr_unet_k_* above; csrc/sdx4_api.h documents the
 * launchers' arguments).  hw is a multiple of 4, the float pointers 16-byte and the frame 4-byte aligned; n is 1 or 2.
 *   nesr_sdx4_k_prepare  sample [n][lc + 3][hw]: channels lc .. lc + 2 = sa (frame [hw][3] u8 / 127.5 - 1) + sb noise [3][hw], channels
 *                        0 .. lc - 1 = sigma latents [lc][hw], which also go to latents_out [lc][hw]
 *   nesr_sdx4_k_step     model [n][lc][hw], latents [lc][hw], the guidance and six HOST coefficients -> latents_out [lc][hw] (may be
 *                        latents) and channels 0 .. lc - 1 of every sample of sample [n][lc + 3][hw]; channels lc .. are left
 */
int nesr_sdx4_k_prepare(const uint8_t* frame_dev, const float* noise_dev, const float* latents_dev, int n, int hw, int lc, float sa, float sb, float sigma,
                        float* sample_dev, float* latents_out_dev, void* hip_stream);
int nesr_sdx4_k_step(const float* model_dev, const float* latents_dev, int n, int hw, int lc, float guidance, const float* coefficients,
                     float* latents_out_dev, float* sample_dev, void* hip_stream);
/*
 * Single-launch entries of the five window kernels (csrc/sdx4_api.h documents the launchers' arguments).  `axes`: eight HOST
 * integers, (n, t, r, a) of the y axis, then of the x axis: the frame's length, the window's, the ramp and the window's origin
 * (the two kernels that normalise ignore a); the blend kernels take them at the output resolution.  Every n, t and a is even, r
 * is below t, the float pointers are 8-byte aligned (blend_finish: 16, and x.n a multiple of 4).
 *   nesr_sdx4_k_window_gather  src [channels][y.n][x.n] -> dst [n][channels][y.t][x.t], every sample the same
 *   nesr_sdx4_k_accumulate     acc [lc][y.n][x.n] += w (model[0] + g (model[1] - model[0])) (n = 2; n = 1: model[0]) of model [n][lc][y.t][x.t]
 *   nesr_sdx4_k_tiled_step     m = acc / S, the DDIM step of nesr_sdx4_k_step on channels 0 .. lc - 1 of frame [lc + 3][y.n][x.n], acc <- 0
 *   nesr_sdx4_k_blend_add      acc [y.n][x.n][3] += w sample [3][y.t][x.t]
 *   nesr_sdx4_k_blend_finish   out [y.n][x.n][3] u8 = rint(clamp(acc / S / 2 + 0.5, 0, 1) 255)
 */
int nesr_sdx4_k_window_gather(const float* src_dev, int n, int channels, const int* axes, float* dst_dev, void* hip_stream);
int nesr_sdx4_k_accumulate(const float* model_dev, int n, int lc, const int* axes, float guidance, float* acc_dev, void* hip_stream);
int nesr_sdx4_k_tiled_step(float* acc_dev, float* frame_dev, int lc, const int* axes, const float* coefficients, void* hip_stream);
int nesr_sdx4_k_blend_add(const float* sample_dev, const int* axes, float* acc_dev, void* hip_stream);
int nesr_sdx4_k_blend_finish(const float* acc_dev, const int* axes, uint8_t* out_dev, void* hip_stream);

const char* nesr_last_error(void);
const char* nesr_version(void);

#ifdef __cplusplus
}
#endif
#endif /* NESR_HIP_H */

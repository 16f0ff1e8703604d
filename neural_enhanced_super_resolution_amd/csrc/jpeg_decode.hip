// Baseline JPEG decoder for gfx950: libjpeg-turbo's default decompressor (JDCT_ISLOW, fancy upsampling, no merged upsampling) pixel
// for pixel (tests/jpeg_decode_ref.py is the specification).  The file's bytes are on the device; the host has parsed the header.
//
// Passes, all on one stream:
//   count      per 4096-byte chunk of the scan: bytes to drop (the 00 of FF 00, both bytes of FF Dn) and restart markers
//   scan       exclusive scan of both counts (one 64-bit word per chunk); the stream's length, the marker count check
//   compact    the unstuffed stream, and the byte at which each restart interval starts in it
//   entropy    with DRI: one restart interval per lane, coefficients at block i Ri per, DC predicted in the lane
//              without: self-synchronising decode.  sync_intra: lane i decodes subsequence i (1024 bits) from the guess (DC next, first
//              block of an MCU), then walks on through i + 1, i + 2, .. of its workgroup until its state at a boundary equals the one
//              recorded there, overwriting the records it passes; rounds are separated by __syncthreads and bounded by the
//              workgroup's subsequence count.  sync_inter: the first lane of each workgroup redoes that from the state the workgroup
//              before it recorded last; launched until no workgroup changed a record (the host reads a 4-byte count), at most once
//              per workgroup.  No workgroup ever waits on another.  Then a scan of the blocks per subsequence, a write pass (DC
//              differences in the DC slot) and a three-kernel prefix sum of the DC differences per component.
//   idct       dequantise, jidctint.c's two passes through an int32 LDS tile of odd pitch, 8-bit samples into component planes
//   colour     h2v2 / h2v1 fancy upsampling read from the planes (the apron comes from the scratch, the IDCT is never redone),
//              YCbCr -> RGB, interleaved store, 4 pixels per lane in three 32-bit stores where the row allows
// Every decode loop advances at least one bit per turn and ends at the stream's length; every coefficient store is guarded by the
// frame's block count; every stream load by the stream's capacity.  A corrupt scan sets bits of the status word.
#include "codec_device.h"
#include "jpeg_decode_kernels.h"
#include "jpeg_tables.h"

namespace nesr {
namespace jpegdec {

namespace {

struct Zigzag {
    uint8_t v[64];
};
constexpr Zigzag make_zigzag() {
    Zigzag z{};
    for (int i = 0; i < 64; ++i) z.v[i] = jpeg::ZIGZAG[i];
    return z;
}
__device__ const Zigzag DZ = make_zigzag();

// ---------------------------------------------------------------------------------------------------------------- scan preparation
__device__ __forceinline__ bool is_rst(int b) { return (b & 0xF8) == 0xD0; }

// lds[1 + i] = byte i of chunk c; lds[0] the byte before it, lds[UNSTUFF_CHUNK + 1] the byte after it; 0 outside the scan
__device__ __forceinline__ void load_chunk(const uint8_t* scan, int64_t n, int64_t c, uint8_t* lds) {
    const int64_t base = c * UNSTUFF_CHUNK - 1;
    for (int i = threadIdx.x; i < UNSTUFF_CHUNK + 2; i += 256) {
        const int64_t at = base + i;
        lds[i] = (at >= 0 && at < n) ? scan[at] : (uint8_t)0;
    }
    __syncthreads();
}

// byte i of the chunk (lds index i + 1): dropped from the stream?  starts a restart marker?
__device__ __forceinline__ void classify(const uint8_t* lds, int i, bool& drop, bool& marker) {
    const int prev = lds[i], b = lds[i + 1], next = lds[i + 2];
    marker = b == 0xFF && is_rst(next);
    drop = marker || (b == 0 && prev == 0xFF) || (is_rst(b) && prev == 0xFF);
}

__global__ __launch_bounds__(256) void jd_count(const uint8_t* scan, int64_t n, uint64_t* chunk) {
    __shared__ uint8_t lds[UNSTUFF_CHUNK + 2];
    __shared__ uint32_t dropped, markers;
    if (threadIdx.x == 0) dropped = markers = 0;
    load_chunk(scan, n, blockIdx.x, lds);
    const int64_t base = (int64_t)blockIdx.x * UNSTUFF_CHUNK;
    uint32_t d = 0, m = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int i = threadIdx.x * 16 + j;
        bool drop, marker;
        classify(lds, i, drop, marker);
        if (base + i < n) {
            d += drop;
            m += marker;
        }
    }
    if (d) atomicAdd(&dropped, d);
    if (m) atomicAdd(&markers, m);
    __syncthreads();
    if (threadIdx.x == 0) chunk[blockIdx.x] = (uint64_t)dropped | ((uint64_t)markers << 32);
}

__global__ __launch_bounds__(1024) void jd_scan_chunks(uint64_t* chunk, int64_t nchunks, int64_t scan_bytes, int64_t nseg, uint32_t* meta, uint32_t* status) {
    __shared__ uint64_t buf[2][1024];
    const uint64_t total = codec::group_scan_1024<uint64_t>(nchunks, buf, [&](int64_t i) { return chunk[i]; }, [&](int64_t i, uint64_t x) { chunk[i] = x; });
    if (threadIdx.x == 0) {
        const uint32_t bytes = (uint32_t)(scan_bytes - (int64_t)(total & 0xFFFFFFFFu));
        meta[0] = bytes;
        meta[1] = (uint32_t)(((uint64_t)bytes * 8 + SUBSEQ_BITS - 1) / SUBSEQ_BITS);
        if ((int64_t)(total >> 32) != nseg - 1) atomicOr(status, ST_RST_COUNT);
    }
}

__global__ __launch_bounds__(256) void jd_compact(const uint8_t* scan, int64_t n, const uint64_t* chunk, uint8_t* stream, int64_t stream_bytes, uint32_t* seg,
                                                   int64_t nseg, uint32_t* status) {
    __shared__ uint8_t lds[UNSTUFF_CHUNK + 2];
    __shared__ uint8_t staged[UNSTUFF_CHUNK];
    __shared__ uint32_t sc[2][256];
    const int tid = threadIdx.x;
    load_chunk(scan, n, blockIdx.x, lds);
    const int64_t base = (int64_t)blockIdx.x * UNSTUFF_CHUNK;
    uint32_t kept = 0, marks = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int i = tid * 16 + j;
        bool drop, marker;
        classify(lds, i, drop, marker);
        if (base + i < n) {
            kept += !drop;
            marks += marker;
        }
    }
    const uint32_t mine = kept | (marks << 16);            // at most 4096 of either per chunk
    int cur = 0;
    sc[0][tid] = mine;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const uint32_t x = sc[cur][tid] + (tid >= d ? sc[cur][tid - d] : 0);
        sc[cur ^ 1][tid] = x;
        cur ^= 1;
        __syncthreads();
    }
    const uint32_t before = sc[cur][tid] - mine;
    const uint32_t chunk_out = sc[cur][255] & 0xFFFF;
    const uint64_t info = chunk[blockIdx.x];
    const int64_t out_base = base - (int64_t)(info & 0xFFFFFFFFu);
    int o = (int)(before & 0xFFFF);
    int64_t k = (int64_t)(info >> 32) + (before >> 16) + 1;          // the interval the next marker starts
    for (int j = 0; j < 16; ++j) {
        const int i = tid * 16 + j;
        if (base + i >= n) break;
        bool drop, marker;
        classify(lds, i, drop, marker);
        if (marker) {
            if (k < nseg) seg[k] = (uint32_t)(out_base + o);
            if ((lds[i + 2] & 7) != (int)((k - 1) & 7)) atomicOr(status, ST_RST_NUMBER);
            ++k;
        }
        if (!drop) staged[o++] = lds[i + 1];
    }
    __syncthreads();
    for (int i = tid; i < (int)chunk_out; i += 256)
        if (out_base + i < stream_bytes) stream[out_base + i] = staged[i];
}

// ---------------------------------------------------------------------------------------------------------------- entropy decoding
constexpr int TABLE_WORDS = (int)(6 * sizeof(nesr_jpeg_huff) / 4);

__device__ __forceinline__ void load_tables(const nesr_jpeg_huff* g, nesr_jpeg_huff* l) {
    const uint32_t* from = reinterpret_cast<const uint32_t*>(g);
    uint32_t* to = reinterpret_cast<uint32_t*>(l);
    for (int i = threadIdx.x; i < TABLE_WORDS; i += blockDim.x) to[i] = from[i];
    __syncthreads();
}

struct Reader {
    const uint32_t* w;
    uint32_t nwords;
    uint32_t base = 0xFFFFFFFEu;    // index of the word in `a` (none yet)
    uint32_t a = 0, b = 0, c = 0;   // words base, base + 1, base + 2 of the stream, most significant bit first; c is loaded one word
                                    // ahead of its use, so its latency hides behind the symbols of the word before
    __device__ __forceinline__ uint32_t load(uint32_t i) const { return i < nwords ? __builtin_bswap32(w[i]) : 0u; }      // 0 past the capacity
    // the 16 bits at bit p
    __device__ __forceinline__ uint32_t peek16(uint32_t p) {
        const uint32_t i = p >> 5;
        if (i != base) {
            if (i == base + 1) {
                a = b;
                b = c;
            } else {
                a = load(i);
                b = load(i + 1);
            }
            c = load(i + 2);
            base = i;
        }
        const uint64_t v = ((uint64_t)a << 32) | b;
        return (uint32_t)(v >> (48 - (p & 31))) & 0xFFFFu;
    }
};

struct State {
    uint32_t p;     // bit of the unstuffed stream
    int z;          // zigzag index of the next coefficient (0: the DC symbol comes next)
    int b;          // block in the MCU
};

__device__ __forceinline__ uint64_t pack(const State& s) { return (uint64_t)s.p | ((uint64_t)s.z << 32) | ((uint64_t)s.b << 40); }
__device__ __forceinline__ State unpack(uint64_t v) { return State{(uint32_t)v, (int)((v >> 32) & 127), (int)((v >> 40) & 15)}; }

struct Shape {
    int ydata, per;   // Y blocks per MCU, blocks per MCU
};

__device__ __forceinline__ int extend(uint32_t x, int size) { return x >= (1u << (size - 1)) ? (int)x : (int)x - (1 << size) + 1; }

// One symbol at s: a Huffman code and its extra bits.  sink(zigzag index, value) for a coefficient; done: the block is complete.
// Advances s.p by at least one bit.  Returns status bits.
template <typename Sink>
__device__ __forceinline__ uint32_t step(State& s, const nesr_jpeg_huff* tabs, Reader& rd, const Shape sh, bool& done, Sink&& sink) {
    const int comp = s.b < sh.ydata ? 0 : s.b - sh.ydata + 1;
    const nesr_jpeg_huff& t = tabs[(s.z == 0 ? 0 : 3) + comp];
    const uint32_t v = rd.peek16(s.p);
    const uint32_t e = t.look[v >> 7];
    uint32_t err = 0;
    int len, sym;
    if (e) {
        len = (int)(e >> 8);
        sym = (int)(e & 255);
    } else {
        len = 10;
        while (len <= 16 && (int)(v >> (16 - len)) > t.maxcode[len]) ++len;
        if (len > 16) {
            err = ST_BAD_CODE;
            len = 16;
            sym = 0;
        } else {
            sym = t.vals[((int)(v >> (16 - len)) + t.valoff[len]) & 255];
        }
    }
    s.p += (uint32_t)len;
    if (s.z == 0) {
        int size = sym;
        if (size > 15) {
            err |= ST_BAD_CODE;
            size &= 15;
        }
        int val = 0;
        if (size) {
            val = extend(rd.peek16(s.p) >> (16 - size), size);
            s.p += (uint32_t)size;
        }
        sink(0, val);
        s.z = 1;
    } else {
        const int run = sym >> 4, size = sym & 15;
        if (size == 0) {
            s.z = run == 15 ? s.z + 16 : 64;
        } else {
            s.z += run;
            if (s.z > 63) {
                err |= ST_RUN;
                s.z = 64;
            } else {
                const int val = extend(rd.peek16(s.p) >> (16 - size), size);
                s.p += (uint32_t)size;
                sink(s.z, val);
                s.z += 1;
            }
        }
    }
    done = s.z >= 64;
    if (done) {
        s.z = 0;
        s.b = s.b + 1 == sh.per ? 0 : s.b + 1;
    }
    return err;
}

// decodes from s up to bit `end`; returns the blocks completed
__device__ __forceinline__ uint32_t run_sub(State& s, uint32_t end, const nesr_jpeg_huff* tabs, Reader& rd, const Shape sh) {
    uint32_t c = 0;
    while (s.p < end) {
        bool done;
        step(s, tabs, rd, sh, done, [](int, int) {});
        c += done;
    }
    return c;
}

__device__ __forceinline__ uint32_t sub_end(uint32_t j, uint32_t total_bits) {
    const uint64_t e = ((uint64_t)j + 1) * SUBSEQ_BITS;
    return e < total_bits ? (uint32_t)e : total_bits;
}

__global__ __launch_bounds__(SUBSEQ_PER_GROUP) void jd_sync_intra(const nesr_jpeg_huff* tables, const uint32_t* stream, uint32_t nwords, const uint32_t* meta,
                                                                   Shape sh, uint64_t* rec, uint32_t* cnt) {
    __shared__ nesr_jpeg_huff tabs[6];
    __shared__ uint64_t lrec[SUBSEQ_PER_GROUP];
    __shared__ uint32_t lcnt[SUBSEQ_PER_GROUP];
    load_tables(tables, tabs);
    Reader rd{stream, nwords};
    const uint32_t total_bits = meta[0] * 8u, nsub = meta[1];
    const int t = threadIdx.x;
    const uint32_t first = blockIdx.x * SUBSEQ_PER_GROUP;
    if (first >= nsub) return;
    const int mine = (int)min((uint32_t)SUBSEQ_PER_GROUP, nsub - first);       // subsequences of this workgroup
    State s{(first + t) * (uint32_t)SUBSEQ_BITS, 0, 0};
    bool active = t < mine;
    if (active) {
        lcnt[t] = run_sub(s, sub_end(first + t, total_bits), tabs, rd, sh);
        lrec[t] = pack(s);
    }
    __syncthreads();
    // round r: lane t decodes subsequence t + r from its own state; lane 0 guessed right (relative to the workgroup's entry), so
    // after round r the records 0 .. r are those of lane 0's path
    for (int r = 1; r < mine; ++r) {
        active = active && t + r < mine;
        if (active) {
            const uint32_t c = run_sub(s, sub_end(first + t + r, total_bits), tabs, rd, sh);
            const uint64_t now = pack(s);
            active = now != lrec[t + r];               // equal: from here on this lane would repeat what lane t + 1 found
            lrec[t + r] = now;
            lcnt[t + r] = c;
        }
        if (__syncthreads_count(active) == 0) break;
    }
    __syncthreads();
    if (t < mine) {
        rec[first + t] = lrec[t];
        cnt[first + t] = lcnt[t];
    }
}

// the first lane of workgroup g >= 1 enters with the state workgroup g - 1 recorded last and corrects its own records until they agree
__global__ __launch_bounds__(64) void jd_sync_inter(const nesr_jpeg_huff* tables, const uint32_t* stream, uint32_t nwords, const uint32_t* meta, Shape sh,
                                                    uint64_t* rec, uint32_t* cnt, uint32_t* unsync) {
    __shared__ nesr_jpeg_huff tabs[6];
    load_tables(tables, tabs);
    Reader rd{stream, nwords};
    const uint32_t total_bits = meta[0] * 8u, nsub = meta[1];
    const uint32_t first = (blockIdx.x + 1) * SUBSEQ_PER_GROUP;
    if (threadIdx.x != 0 || first >= nsub) return;
    const uint32_t last = min(nsub, first + SUBSEQ_PER_GROUP);
    State s = unpack(rec[first - 1]);
    bool changed = false;
    for (uint32_t j = first; j < last; ++j) {
        const uint32_t c = run_sub(s, sub_end(j, total_bits), tabs, rd, sh);
        const uint64_t now = pack(s);
        const bool same = now == rec[j];
        changed = changed || !same || c != cnt[j];
        rec[j] = now;
        cnt[j] = c;
        if (same) break;
    }
    if (changed) atomicAdd(unsync, 1u);
}

__global__ __launch_bounds__(1024) void jd_scan_counts(uint32_t* cnt, uint32_t* meta, int64_t nblocks, uint32_t* status) {
    __shared__ uint32_t buf[2][1024];
    const uint32_t total = codec::group_scan_1024<uint32_t>((int64_t)meta[1], buf, [&](int64_t i) { return cnt[i]; }, [&](int64_t i, uint32_t x) { cnt[i] = x; });
    if (threadIdx.x == 0) {
        meta[2] = total;
        if ((int64_t)total < nblocks) atomicOr(status, ST_EARLY);
        // the 1-bits that pad the last byte may read as the start of one more block
        if ((int64_t)total > nblocks + 1) atomicOr(status, ST_EXTRA);
    }
}

__global__ __launch_bounds__(SUBSEQ_PER_GROUP) void jd_write(const nesr_jpeg_huff* tables, const uint32_t* stream, uint32_t nwords, const uint32_t* meta, Shape sh,
                                                              const uint64_t* rec, const uint32_t* first_block, int16_t* coef, int64_t nblocks, uint32_t* status) {
    __shared__ nesr_jpeg_huff tabs[6];
    __shared__ uint8_t zz[64];                             // the zigzag in LDS: a coefficient's address must not wait for global memory
    if (threadIdx.x < 64) zz[threadIdx.x] = DZ.v[threadIdx.x];
    load_tables(tables, tabs);
    Reader rd{stream, nwords};
    const uint32_t total_bits = meta[0] * 8u, nsub = meta[1];
    const uint32_t j = blockIdx.x * SUBSEQ_PER_GROUP + threadIdx.x;
    if (j >= nsub) return;
    State s = j ? unpack(rec[j - 1]) : State{0, 0, 0};
    int64_t blk = first_block[j];
    const uint32_t end = sub_end(j, total_bits);
    uint32_t err = 0;
    while (s.p < end) {
        bool done;
        const uint32_t e = step(s, tabs, rd, sh, done, [&](int z, int val) {
            if (blk < nblocks) coef[blk * 64 + zz[z]] = (int16_t)val;
        });
        if (blk < nblocks) err |= e;
        blk += done;
    }
    if (err) atomicOr(status, err);
}

// one restart interval per lane: the state at its start is known, and so is its first block
__global__ __launch_bounds__(DRI_LANES) void jd_decode_dri(const nesr_jpeg_huff* tables, const uint32_t* stream, uint32_t nwords, const uint32_t* meta, Shape sh,
                                                           const uint32_t* seg, int64_t nseg, int64_t ri, int64_t nmcu, int16_t* coef, int64_t nblocks,
                                                           uint32_t* status) {
    __shared__ nesr_jpeg_huff tabs[6];
    __shared__ uint8_t zz[64];
    if (threadIdx.x < 64) zz[threadIdx.x] = DZ.v[threadIdx.x];
    load_tables(tables, tabs);
    Reader rd{stream, nwords};
    const uint32_t bytes = meta[0];
    const int64_t sgm = (int64_t)blockIdx.x * DRI_LANES + threadIdx.x;
    if (sgm >= nseg) return;
    const uint32_t start = min(sgm ? seg[sgm] : 0u, bytes);
    const uint32_t stop = max(start, min(sgm + 1 < nseg ? seg[sgm + 1] : bytes, bytes));
    State s{start * 8u, 0, 0};
    const uint32_t end = stop * 8u;
    int64_t blk = sgm * ri * sh.per;
    const int64_t blk_end = min((sgm + 1) * ri, nmcu) * sh.per;
    int pred0 = 0, pred1 = 0, pred2 = 0;
    uint32_t err = 0;
    while (blk < blk_end && s.p < end) {
        const int comp = s.b < sh.ydata ? 0 : s.b - sh.ydata + 1;
        bool done;
        err |= step(s, tabs, rd, sh, done, [&](int z, int val) {
            if (z == 0) {
                int& pred = comp == 0 ? pred0 : (comp == 1 ? pred1 : pred2);
                pred += val;
                val = pred;
            }
            if (blk < nblocks) coef[blk * 64 + zz[z]] = (int16_t)val;
        });
        blk += done;
    }
    if (blk < blk_end || s.p > end) err |= ST_EARLY;
    if (err) atomicOr(status, err);
}

// ---------------------------------------------------------------------------------------------------------------- DC prediction
// The DC slots hold differences; each component's DC is the running sum over its blocks in scan order.  One MCU per lane.
__device__ __forceinline__ void mcu_sums(const int16_t* coef, int64_t m, int64_t nmcu, Shape sh, int v[3]) {
    v[0] = v[1] = v[2] = 0;
    if (m >= nmcu) return;
    const int16_t* p = coef + m * sh.per * 64;
    for (int k = 0; k < sh.ydata; ++k) v[0] += p[k * 64];
    if (sh.per > sh.ydata) {
        v[1] = p[sh.ydata * 64];
        v[2] = p[(sh.ydata + 1) * 64];
    }
}

__global__ __launch_bounds__(DC_GROUP) void jd_dc_sums(const int16_t* coef, int64_t nmcu, Shape sh, int32_t* dc) {
    __shared__ int total[3];
    if (threadIdx.x < 3) total[threadIdx.x] = 0;
    __syncthreads();
    int v[3];
    mcu_sums(coef, (int64_t)blockIdx.x * DC_GROUP + threadIdx.x, nmcu, sh, v);
    for (int c = 0; c < 3; ++c)
        if (v[c]) atomicAdd(&total[c], v[c]);
    __syncthreads();
    if (threadIdx.x < 3) dc[blockIdx.x * 3 + threadIdx.x] = total[threadIdx.x];
}

__global__ __launch_bounds__(1024) void jd_dc_scan(int32_t* dc, int64_t groups) {
    __shared__ int32_t buf[2][1024];
    for (int c = 0; c < 3; ++c)             // dc[3 g + c]: one scan per component
        codec::group_scan_1024<int32_t>(groups, buf, [&](int64_t i) { return dc[3 * i + c]; }, [&](int64_t i, int32_t x) { dc[3 * i + c] = x; });
}

__global__ __launch_bounds__(DC_GROUP) void jd_dc_apply(int16_t* coef, int64_t nmcu, Shape sh, const int32_t* dc) {
    __shared__ int sc[2][3][DC_GROUP];
    const int tid = threadIdx.x;
    const int64_t m = (int64_t)blockIdx.x * DC_GROUP + tid;
    int v[3];
    mcu_sums(coef, m, nmcu, sh, v);
    int cur = 0;
    for (int c = 0; c < 3; ++c) sc[0][c][tid] = v[c];
    __syncthreads();
    for (int d = 1; d < DC_GROUP; d <<= 1) {
        for (int c = 0; c < 3; ++c) sc[cur ^ 1][c][tid] = sc[cur][c][tid] + (tid >= d ? sc[cur][c][tid - d] : 0);
        cur ^= 1;
        __syncthreads();
    }
    if (m >= nmcu) return;
    int run[3];
    for (int c = 0; c < 3; ++c) run[c] = dc[blockIdx.x * 3 + c] + sc[cur][c][tid] - v[c];
    int16_t* p = coef + m * sh.per * 64;
    for (int k = 0; k < sh.per; ++k) {
        const int c = k < sh.ydata ? 0 : k - sh.ydata + 1;
        run[c] += p[k * 64];
        p[k * 64] = (int16_t)run[c];
    }
}

// ---------------------------------------------------------------------------------------------------------------- reconstruction
// jidctint.c, one 8-point pass, descaled by N bits
template <int N>
__device__ __forceinline__ void idct8(const int d[8], int o[8]) {
    constexpr int R = 1 << (N - 1);
    int z2 = d[2], z3 = d[6];
    int z1 = (z2 + z3) * 4433;
    const int tmp2 = z1 - z3 * 15137, tmp3 = z1 + z2 * 6270;
    const int tmp0 = (int)((unsigned)(d[0] + d[4]) << 13), tmp1 = (int)((unsigned)(d[0] - d[4]) << 13);
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    int t0 = d[7], t1 = d[5], t2 = d[3], t3 = d[1];
    z1 = t0 + t3;
    z2 = t1 + t2;
    z3 = t0 + t2;
    int z4 = t1 + t3;
    const int z5 = (z3 + z4) * 9633;
    t0 *= 2446;
    t1 *= 16819;
    t2 *= 25172;
    t3 *= 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    t0 += z1 + z3;
    t1 += z2 + z4;
    t2 += z2 + z3;
    t3 += z1 + z4;
    o[0] = (tmp10 + t3 + R) >> N;
    o[7] = (tmp10 - t3 + R) >> N;
    o[1] = (tmp11 + t2 + R) >> N;
    o[6] = (tmp11 - t2 + R) >> N;
    o[2] = (tmp12 + t1 + R) >> N;
    o[5] = (tmp12 - t1 + R) >> N;
    o[3] = (tmp13 + t0 + R) >> N;
    o[4] = (tmp13 - t0 + R) >> N;
}

struct ReconArgs {
    const int16_t* coef;
    int64_t nblocks;
    uint16_t q[3][64];
    int ydata, per, hs, mcus_x;
    uint8_t *y, *cb, *cr;
    int ypitch, cpitch;
};

constexpr int WS_PITCH = 72;               // int32 per block between the IDCT passes: rows of 9 (odd: no bank conflicts either way)

__global__ __launch_bounds__(256) void jd_idct(const ReconArgs a) {
    __shared__ int ws[RECON_BLOCKS * WS_PITCH];
    const int tid = threadIdx.x;
    const int b = tid >> 3, r = tid & 7;
    const int64_t n = (int64_t)blockIdx.x * RECON_BLOCKS + b;
    const bool valid = n < a.nblocks;
    int comp = 0;
    uint8_t* out = nullptr;
    if (valid) {
        const int64_t m = n / a.per;
        const int k = (int)(n - m * a.per);
        const int my = (int)(m / a.mcus_x), mx = (int)(m - (int64_t)my * a.mcus_x);
        if (k < a.ydata) {
            const int by = my * (a.ydata / a.hs) + k / a.hs, bx = mx * a.hs + k % a.hs;
            out = a.y + ((int64_t)by * 8 + r) * a.ypitch + bx * 8;
        } else {
            comp = k - a.ydata + 1;
            out = (comp == 1 ? a.cb : a.cr) + ((int64_t)my * 8 + r) * a.cpitch + mx * 8;
        }
        const uint4 v = reinterpret_cast<const uint4*>(a.coef + n * 64)[r];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) ws[b * WS_PITCH + r * 9 + i] = (int)(int16_t)(w[i >> 1] >> ((i & 1) * 16)) * (int)a.q[comp][r * 8 + i];
    }
    __syncthreads();
    int d[8], o[8];
    if (valid) {                                           // columns: lane (block, column r)
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = ws[b * WS_PITCH + i * 9 + r];
        idct8<11>(d, o);
#pragma unroll
        for (int i = 0; i < 8; ++i) ws[b * WS_PITCH + i * 9 + r] = o[i];
    }
    __syncthreads();
    if (valid) {                                           // rows: lane (block, row r)
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = ws[b * WS_PITCH + r * 9 + i];
        idct8<18>(d, o);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            lo |= (uint32_t)min(max(o[i] + 128, 0), 255) << (8 * i);
            hi |= (uint32_t)min(max(o[i + 4] + 128, 0), 255) << (8 * i);
        }
        *reinterpret_cast<uint2*>(out) = make_uint2(lo, hi);          // planes and pitches are multiples of 8
    }
}

// ---------------------------------------------------------------------------------------------------------------- upsampling, colour
struct ColorArgs {
    const uint8_t *y, *cb, *cr;
    int ypitch, cpitch;
    int H, W, C, hs, vs, bgr;
    uint8_t* dst;
    int64_t stride;
};

// jdsample.c: the chroma sample at pixel (x, y).  cw x ch real chroma samples; fancy upsampling only when cw > 2, as libjpeg chooses.
__device__ __forceinline__ int chroma_at(const uint8_t* p, int pitch, int x, int y, int hs, int vs, int cw, int ch) {
    if (hs == 1) return p[(int64_t)y * pitch + x];
    const int c = x >> 1;
    if (vs == 1) {
        const uint8_t* row = p + (int64_t)y * pitch;
        const int t = row[c];
        if (cw <= 2) return t;
        if (x & 1) return c == cw - 1 ? t : (3 * t + row[c + 1] + 2) >> 2;
        return c == 0 ? t : (3 * t + row[c - 1] + 1) >> 2;
    }
    const int cy = y >> 1;
    const uint8_t* near = p + (int64_t)cy * pitch;
    if (cw <= 2) return near[c];
    const uint8_t* far = p + (int64_t)((y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0)) * pitch;
    const int cur = 3 * near[c] + far[c];
    if (x & 1) return (3 * cur + (c == cw - 1 ? cur : 3 * near[c + 1] + far[c + 1]) + 7) >> 4;
    return (3 * cur + (c == 0 ? cur : 3 * near[c - 1] + far[c - 1]) + 8) >> 4;
}

__device__ __forceinline__ uint32_t clamp8(int v) { return (uint32_t)min(max(v, 0), 255); }

__global__ __launch_bounds__(256) void jd_color(const ColorArgs a) {
    const int x0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4;
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x0 >= a.W || y >= a.H) return;
    const int npx = min(4, a.W - x0);
    uint8_t px[12];
    const int cw = (a.W + a.hs - 1) / a.hs, ch = (a.H + a.vs - 1) / a.vs;
    for (int i = 0; i < npx; ++i) {
        const int x = x0 + i;
        const int yy = a.y[(int64_t)y * a.ypitch + x];
        if (a.C == 1) {
            px[i] = (uint8_t)yy;
            continue;
        }
        const int cb = chroma_at(a.cb, a.cpitch, x, y, a.hs, a.vs, cw, ch) - 128;
        const int cr = chroma_at(a.cr, a.cpitch, x, y, a.hs, a.vs, cw, ch) - 128;
        const uint32_t r = clamp8(yy + ((91881 * cr + 32768) >> 16));
        const uint32_t g = clamp8(yy + ((-22554 * cb - 46802 * cr + 32768) >> 16));
        const uint32_t bl = clamp8(yy + ((116130 * cb + 32768) >> 16));
        px[3 * i] = (uint8_t)(a.bgr ? bl : r);
        px[3 * i + 1] = (uint8_t)g;
        px[3 * i + 2] = (uint8_t)(a.bgr ? r : bl);
    }
    uint8_t* out = a.dst + (int64_t)y * a.stride + (int64_t)x0 * a.C;
    const int nbytes = npx * a.C;
    if (npx == 4 && (reinterpret_cast<uintptr_t>(out) & 3) == 0) {
        uint32_t* o32 = reinterpret_cast<uint32_t*>(out);
        for (int i = 0; i < a.C; ++i) o32[i] = (uint32_t)px[4 * i] | ((uint32_t)px[4 * i + 1] << 8) | ((uint32_t)px[4 * i + 2] << 16) | ((uint32_t)px[4 * i + 3] << 24);
    } else {
        for (int i = 0; i < nbytes; ++i) out[i] = px[i];
    }
}

}  // namespace

hipError_t launch_decode(const Plan& p, const DecodeArgs& a, hipStream_t s, int* rounds, int* launches) {
    hipError_t e;
    int nl = 0, nr = 0;
    if ((e = hipMemsetAsync(a.status, 0, 4, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(a.meta, 0, 256, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(a.seg, 0, (size_t)p.nseg * 4, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(a.stream, 0, (size_t)p.stream_words * 4, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(a.coef, 0, (size_t)p.nblocks * 128, s)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(a.tables, a.tables_host, 6 * sizeof(nesr_jpeg_huff), hipMemcpyHostToDevice, s)) != hipSuccess) return e;
    const Shape sh{p.per == 1 ? 1 : p.hs * p.vs, p.per};
    const uint32_t nwords = (uint32_t)p.stream_words;
    hipLaunchKernelGGL(jd_count, dim3((unsigned)p.nchunks), dim3(256), 0, s, a.scan, p.scan_bytes, a.chunk);
    hipLaunchKernelGGL(jd_scan_chunks, dim3(1), dim3(1024), 0, s, a.chunk, p.nchunks, p.scan_bytes, p.nseg, a.meta, a.status);
    hipLaunchKernelGGL(jd_compact, dim3((unsigned)p.nchunks), dim3(256), 0, s, a.scan, p.scan_bytes, a.chunk, reinterpret_cast<uint8_t*>(a.stream),
                       p.stream_words * 4, a.seg, p.nseg, a.status);
    nl += 3;
    if (p.ri > 0) {
        hipLaunchKernelGGL(jd_decode_dri, dim3((unsigned)((p.nseg + DRI_LANES - 1) / DRI_LANES)), dim3(DRI_LANES), 0, s, a.tables, a.stream, nwords, a.meta, sh, a.seg,
                           p.nseg, (int64_t)p.ri, p.nmcu, a.coef, p.nblocks, a.status);
        nl += 1;
    } else {
        hipLaunchKernelGGL(jd_sync_intra, dim3((unsigned)p.ngroups), dim3(SUBSEQ_PER_GROUP), 0, s, a.tables, a.stream, nwords, a.meta, sh, a.rec, a.cnt);
        nl += 1;
        // each launch makes at least one more workgroup's entry state final, so ngroups launches always suffice
        for (int64_t it = 0; p.ngroups > 1 && it < p.ngroups; ++it) {
            uint32_t unsync = 0;
            if ((e = hipMemsetAsync(a.meta + 16, 0, 4, s)) != hipSuccess) return e;
            hipLaunchKernelGGL(jd_sync_inter, dim3((unsigned)(p.ngroups - 1)), dim3(64), 0, s, a.tables, a.stream, nwords, a.meta, sh, a.rec, a.cnt, a.meta + 16);
            if ((e = hipMemcpyAsync(&unsync, a.meta + 16, 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
            if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
            ++nr;
            ++nl;
            if (unsync == 0) break;
        }
        hipLaunchKernelGGL(jd_scan_counts, dim3(1), dim3(1024), 0, s, a.cnt, a.meta, p.nblocks, a.status);
        hipLaunchKernelGGL(jd_write, dim3((unsigned)p.ngroups), dim3(SUBSEQ_PER_GROUP), 0, s, a.tables, a.stream, nwords, a.meta, sh, a.rec, a.cnt, a.coef, p.nblocks,
                           a.status);
        hipLaunchKernelGGL(jd_dc_sums, dim3((unsigned)p.dc_groups), dim3(DC_GROUP), 0, s, a.coef, p.nmcu, sh, a.dc);
        hipLaunchKernelGGL(jd_dc_scan, dim3(1), dim3(1024), 0, s, a.dc, p.dc_groups);
        hipLaunchKernelGGL(jd_dc_apply, dim3((unsigned)p.dc_groups), dim3(DC_GROUP), 0, s, a.coef, p.nmcu, sh, a.dc);
        nl += 5;
    }
    ReconArgs r{};
    r.coef = a.coef;
    r.nblocks = p.nblocks;
    for (int c = 0; c < 3; ++c)
        for (int i = 0; i < 64; ++i) r.q[c][i] = a.q[c][i];
    r.ydata = sh.ydata;
    r.per = p.per;
    r.hs = p.per == 1 ? 1 : p.hs;
    r.mcus_x = p.mcus_x;
    r.y = a.y;
    r.cb = a.cb;
    r.cr = a.cr;
    r.ypitch = p.ypitch;
    r.cpitch = p.cpitch;
    hipLaunchKernelGGL(jd_idct, dim3((unsigned)((p.nblocks + RECON_BLOCKS - 1) / RECON_BLOCKS)), dim3(256), 0, s, r);
    ColorArgs c{a.y, a.cb, a.cr, p.ypitch, p.cpitch, p.H, p.W, p.C, p.C == 1 ? 1 : p.hs, p.C == 1 ? 1 : p.vs, a.bgr, a.dst, a.dst_stride};
    // blockIdx.y carries rows of 4: at most 65535 / 4 + 1, within the grid limit
    hipLaunchKernelGGL(jd_color, dim3((p.W + 255) / 256, (p.H + 3) / 4), dim3(256), 0, s, c);
    nl += 2;
    if (rounds) *rounds = nr;
    if (launches) *launches = nl;
    return hipGetLastError();
}

}  // namespace jpegdec
}  // namespace nesr

// Lossless PNG encoder for gfx950 (tests/png_ref.py is the specification, byte for byte): adaptive row filter from raw neighbours,
// deflate in independent chunks of 32768 filtered bytes with distance-1 matches in closed form, one block and one IDAT per chunk.
//
// Passes, all on one stream, nothing returns to the host between them:
//   filter   a workgroup per row: the five candidates' costs by reduction, the winner's type byte and filtered bytes into the scratch;
//            channel flip (BGR frames) and byte swap (16 bit) are folded into the read; a row-strided source is taken as it is
//   chunk    a workgroup per chunk, the chunk in LDS: run starts and their scans, token histogram and Adler partial sums, code
//            lengths / code-length code / the three costs / BTYPE by one lane, token bit lengths and their scan, LSB-first packing into
//            an LDS image of the IDAT, the sync marker, the framing and its CRC-32; the IDAT goes to the chunk's slot, its size is kept
//   scan     exclusive scan of the IDAT sizes, 64-bit, one workgroup with a carry
//   gather   slots to `out` behind the head at their offsets, dword stores where `out` allows
//   finish   head, Adler-32 across the chunks, the tail IDAT, IEND, the length and status words
// No pass writes out[i] for i >= out_cap.
#include "codec_device.h"
#include "png_kernels.h"

namespace nesr {
namespace png {

namespace {

constexpr int THREADS = 256;
constexpr int SEG = CHUNK / THREADS;               // 128 bytes of the chunk per lane
constexpr int DATA_WORDS = CHUNK / 4 + CHUNK / 128;  // the chunk in LDS, a pad word after every 32: lane t's segment starts in bank t
constexpr int OUT_BYTES = 32832;                   // LDS image of the IDAT: >= SLOT, a multiple of 64
constexpr int CRC_PIECE = 144;                     // bytes per lane of the CRC: 256 * 144 >= 4 + CHUNK + 10
constexpr size_t CHUNK_LDS = (size_t)DATA_WORDS * 4 + OUT_BYTES;

// ---------------------------------------------------------------------------------------------------------------- CRC-32
constexpr uint32_t CRC_POLY = 0xEDB88320u;

struct CrcTable {
    uint32_t t[256];
};
constexpr CrcTable make_crc_table() {
    CrcTable c{};
    for (uint32_t i = 0; i < 256; ++i) {
        uint32_t v = i;
        for (int k = 0; k < 8; ++k) v = (v & 1) ? (v >> 1) ^ CRC_POLY : v >> 1;
        c.t[i] = v;
    }
    return c;
}
// a * b mod P, polynomials bit-reflected (x^0 is bit 31)
constexpr __host__ __device__ uint32_t mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1) ? (b >> 1) ^ CRC_POLY : b >> 1;
    }
    return p;
}
// x^(8 * CRC_PIECE * 2^l) mod P for the levels of the combine tree
struct CrcShift {
    uint32_t x[8];
};
constexpr CrcShift make_crc_shift() {
    CrcShift s{};
    uint32_t v = 1u << 30;                             // x^1
    for (int i = 0; i < 3; ++i) v = mulmod(v, v);      // x^8
    uint32_t p = 1u << 31;                             // x^0
    for (int i = 0; i < CRC_PIECE; ++i) p = mulmod(p, v);
    for (int l = 0; l < 8; ++l) {
        s.x[l] = p;
        p = mulmod(p, p);
    }
    return s;
}
__device__ const CrcTable CRC_TABLE = make_crc_table();
__device__ const CrcShift CRC_SHIFT = make_crc_shift();

__device__ __forceinline__ uint32_t crc_bytes(const uint8_t* p, int n) {      // a whole small message, by one lane
    uint32_t c = 0xFFFFFFFFu;
    for (int i = 0; i < n; ++i) c = CRC_TABLE.t[(c ^ p[i]) & 255] ^ (c >> 8);
    return ~c;
}

// ---------------------------------------------------------------------------------------------------------------- filter
struct FilterArgs {
    const uint8_t* src;
    int64_t stride;
    int W, C, bps, flip;
    int64_t row;                                   // bytes of a filtered row
    uint8_t* filt;
};

__device__ __forceinline__ int paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// byte k of pixel p as the file holds it: R G B (A), big-endian samples
__device__ __forceinline__ int file_byte(const uint8_t* line, int p, int k, int C, int bps, int flip) {
    int ch = bps == 2 ? k >> 1 : k;
    const int lo = bps == 2 ? 1 - (k & 1) : 0;     // the frame's samples are little-endian
    if (flip && ch < 3) ch = 2 - ch;
    return line[((int64_t)p * C + ch) * bps + lo];
}

__global__ __launch_bounds__(THREADS) void png_filter(const FilterArgs a) {
    __shared__ uint32_t cost[5];
    __shared__ int winner;
    const int y = blockIdx.x, tid = threadIdx.x;
    const int bpp = a.C * a.bps;
    const uint8_t* cur = a.src + (int64_t)y * a.stride;
    const uint8_t* up = y ? cur - a.stride : nullptr;
    if (tid < 5) cost[tid] = 0;
    __syncthreads();
    uint32_t sum[5] = {0, 0, 0, 0, 0};
    for (int p = tid; p < a.W; p += THREADS) {
        for (int k = 0; k < bpp; ++k) {
            const int x = file_byte(cur, p, k, a.C, a.bps, a.flip);
            const int l = p ? file_byte(cur, p - 1, k, a.C, a.bps, a.flip) : 0;
            const int u = up ? file_byte(up, p, k, a.C, a.bps, a.flip) : 0;
            const int ul = (up && p) ? file_byte(up, p - 1, k, a.C, a.bps, a.flip) : 0;
            const int v[5] = {x, (x - l) & 255, (x - u) & 255, (x - ((l + u) >> 1)) & 255, (x - paeth(l, u, ul)) & 255};
#pragma unroll
            for (int t = 0; t < 5; ++t) sum[t] += (uint32_t)min(v[t], 256 - v[t]);
        }
    }
#pragma unroll
    for (int t = 0; t < 5; ++t) atomicAdd(&cost[t], sum[t]);                  // integers: any order gives the same sum
    __syncthreads();
    if (tid == 0) {
        int best = 0;
        for (int t = 1; t < 5; ++t)
            if (cost[t] < cost[best]) best = t;                              // ties: the lowest type
        winner = best;
        a.filt[(int64_t)y * a.row] = (uint8_t)best;
    }
    __syncthreads();
    const int type = winner;
    uint8_t* dst = a.filt + (int64_t)y * a.row + 1;
    for (int p = tid; p < a.W; p += THREADS) {
        for (int k = 0; k < bpp; ++k) {
            const int x = file_byte(cur, p, k, a.C, a.bps, a.flip);
            const int l = p ? file_byte(cur, p - 1, k, a.C, a.bps, a.flip) : 0;
            const int u = up ? file_byte(up, p, k, a.C, a.bps, a.flip) : 0;
            const int ul = (up && p) ? file_byte(up, p - 1, k, a.C, a.bps, a.flip) : 0;
            const int pred = type == 0 ? 0 : (type == 1 ? l : (type == 2 ? u : (type == 3 ? (l + u) >> 1 : paeth(l, u, ul))));
            dst[(int64_t)p * bpp + k] = (uint8_t)(x - pred);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- chunk
// byte i of the chunk in the padded LDS image
__device__ __forceinline__ int at(const uint8_t* data, int i) { return data[(((i >> 2) + (i >> 7)) << 2) + (i & 3)]; }

// The tokens of the run [s, s + R) of value v whose first byte lies in [lo, hi), in order: sink(symbol, extra value, extra bits, match)
template <typename Sink>
__device__ __forceinline__ void run_tokens(int s, int R, int v, int lo, int hi, Sink&& sink) {
    if (lo == s) sink(v, 0, 0, false);
    const int r = R - 1, full = r / 258, rem = r - full * 258;
    for (int k = lo <= s + 1 ? 0 : (lo - s - 1 + 257) / 258; k < full && s + 1 + 258 * k < hi; ++k) sink(285, 0, 0, true);
    const int rs = s + 1 + 258 * full;
    if (rem >= 3) {
        if (rs >= lo && rs < hi) {
            int sym, ev, eb;
            length_symbol(rem, sym, ev, eb);
            sink(sym, ev, eb, true);
        }
    } else {
        for (int j = 0; j < rem; ++j)
            if (rs + j >= lo && rs + j < hi) sink(v, 0, 0, false);
    }
}

// The tokens that start in [seg0, seg1).  s0: the start of the run that holds seg0; after: the first run start at or behind seg1.
template <typename Sink>
__device__ __forceinline__ void walk(const uint8_t* data, int seg0, int seg1, int s0, int after, Sink&& sink) {
    int i = seg0, s = s0;
    while (i < seg1) {
        int j = i + 1;
        while (j < seg1 && at(data, j) == at(data, j - 1)) ++j;
        const int e = j < seg1 ? j : after;
        const int hi = e < seg1 ? e : seg1;
        run_tokens(s, e - s, at(data, s), i, hi, sink);
        i = hi;
        s = e;
    }
}

struct BitWriter {                                 // LSB first, into zeroed LDS words that neighbours may share
    uint32_t* out;
    uint32_t word;
    uint64_t acc;
    int n;
    __device__ __forceinline__ BitWriter(uint32_t* o, uint32_t pos) : out(o), word(pos >> 5), acc(0), n((int)(pos & 31)) {}
    __device__ __forceinline__ void put(uint32_t v, int length) {            // length <= 32
        acc |= (uint64_t)v << n;
        n += length;
        if (n >= 32) {
            atomicOr(out + word, (uint32_t)acc);
            acc >>= 32;
            n -= 32;
            ++word;
        }
    }
    __device__ __forceinline__ void finish() {
        if (n > 0) atomicOr(out + word, (uint32_t)acc);
    }
};

struct ChunkShared {
    uint32_t hist[MAX_SYMS];
    uint32_t clhist[32];
    uint32_t scan[2][THREADS];
    int first[2][THREADS], last[2][THREADS];
    uint32_t crc[THREADS];
    uint32_t crc_table[256];
    uint16_t codes[MAX_SYMS];
    uint8_t lens[MAX_SYMS];
    uint8_t seq[MAX_SYMS];
    uint8_t cl[32];
    HuffWork work;
    unsigned long long s1, s2;
    uint32_t nmatch, used;
    int btype, dist_bits;
    uint32_t header_bits;
};

struct ChunkArgs {
    const uint8_t* filt;
    int64_t N, nchunks;
    uint8_t* slot;
    uint64_t* size;
    uint64_t* adler;
};

__global__ __launch_bounds__(THREADS) void png_chunk(const ChunkArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    __shared__ ChunkShared sh;
    uint8_t* data = lds;
    uint32_t* data32 = reinterpret_cast<uint32_t*>(lds);
    uint8_t* out8 = lds + (size_t)DATA_WORDS * 4;
    uint32_t* out32 = reinterpret_cast<uint32_t*>(out8);
    const int tid = threadIdx.x;
    const int64_t c = blockIdx.x;
    const int n = (int)min((int64_t)CHUNK, a.N - c * CHUNK);
    const bool final_chunk = c == a.nchunks - 1;

    // the chunk (the scratch is readable up to the next multiple of 16), zeroed tables and IDAT image
    const uint4* from = reinterpret_cast<const uint4*>(a.filt + c * CHUNK);
    for (int q = tid; q * 16 < n; q += THREADS) {
        const uint4 v = from[q];
        uint32_t* d = data32 + 4 * q + (q >> 3);
        d[0] = v.x;
        d[1] = v.y;
        d[2] = v.z;
        d[3] = v.w;
    }
    for (int i = tid; i < OUT_BYTES / 4; i += THREADS) out32[i] = 0;
    for (int i = tid; i < MAX_SYMS; i += THREADS) sh.hist[i] = 0;
    sh.crc_table[tid] = CRC_TABLE.t[tid];
    if (tid < 32) sh.clhist[tid] = 0;
    if (tid == 0) {
        sh.s1 = sh.s2 = 0;
        sh.nmatch = sh.used = 0;
    }
    __syncthreads();

    // run starts: the last one in each lane's segment scanned forwards (max), the first one scanned backwards (min)
    const int seg0 = tid * SEG, seg1 = min(seg0 + SEG, n);
    {
        int first = n, last = -1;
        for (int i = seg0; i < seg1; ++i) {
            if (i == 0 || at(data, i) != at(data, i - 1)) {
                if (last < 0) first = i;
                last = i;
            }
        }
        sh.first[0][tid] = first;
        sh.last[0][tid] = last;
    }
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < THREADS; d <<= 1) {
        const int l = max(sh.last[cur][tid], tid >= d ? sh.last[cur][tid - d] : -1);
        const int f = min(sh.first[cur][tid], tid + d < THREADS ? sh.first[cur][tid + d] : n);
        sh.last[cur ^ 1][tid] = l;
        sh.first[cur ^ 1][tid] = f;
        cur ^= 1;
        __syncthreads();
    }
    int s0 = 0, after = n;
    if (seg0 < n) {
        s0 = (seg0 == 0 || at(data, seg0) != at(data, seg0 - 1)) ? seg0 : sh.last[cur][tid - 1];
        after = tid + 1 < THREADS ? sh.first[cur][tid + 1] : n;
    }

    // token histogram, Adler partial sums
    {
        uint32_t matches = 0;
        walk(data, seg0, seg1, s0, after, [&](int sym, int, int, bool m) {
            atomicAdd(&sh.hist[sym], 1u);
            matches += m ? 1u : 0u;
        });
        if (matches) atomicAdd(&sh.nmatch, matches);
        if (seg0 < seg1) {
            uint32_t s1 = 0, s2 = 0;
            for (int i = seg0; i < seg1; ++i) {
                const uint32_t d = (uint32_t)at(data, i);
                s1 += d;
                s2 += (uint32_t)(seg1 - i) * d;
            }
            atomicAdd(&sh.s1, (unsigned long long)s1);                       // integers: any order gives the same sum
            atomicAdd(&sh.s2, (unsigned long long)s2 + (unsigned long long)(n - seg1) * s1);
        }
    }
    __syncthreads();
    if (tid == 0) sh.hist[256] = 1;
    __syncthreads();

    // the used symbols ranked by (count, symbol): the sort of png_ref.code_lengths
    for (int s = tid; s < NLIT; s += THREADS) {
        const uint32_t mine = sh.hist[s];
        if (!mine) continue;
        int rank = 0;
        for (int j = 0; j < NLIT; ++j) {
            const uint32_t o = sh.hist[j];
            rank += (o && (o < mine || (o == mine && j < s))) ? 1 : 0;
        }
        sh.work.order[rank] = (uint16_t)s;
        atomicAdd(&sh.used, 1u);
    }
    __syncthreads();

    // one lane: the codes, the three costs, BTYPE, the block header
    if (tid == 0) {
        const uint32_t nmatch = sh.nmatch;
        uint8_t* ll = sh.lens;
        code_lengths_sorted(sh.hist, (int)sh.used, NLIT, 15, ll, sh.work);
        ll[286] = ll[287] = 0;
        const int dl = nmatch ? 1 : 0;
        int hlit = 257;
        for (int s = 257; s < NLIT; ++s)
            if (ll[s]) hlit = s + 1;
        for (int s = 0; s < hlit; ++s) sh.seq[s] = ll[s];
        sh.seq[hlit] = (uint8_t)dl;
        uint32_t rle_extra = 0;
        rle_lengths(sh.seq, hlit + 1, [&](int s, int, int eb) {
            ++sh.clhist[s];
            rle_extra += (uint32_t)eb;
        });
        const int m2 = sort_used(sh.clhist, NCL, sh.work);
        code_lengths_sorted(sh.clhist, m2, NCL, 7, sh.cl, sh.work);
        const int order[NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        int hclen = 4;
        for (int i = 4; i < NCL; ++i)
            if (sh.cl[order[i]]) hclen = i + 1;
        uint32_t extra = 0, fixed_bits = 3 + 5 * nmatch, dyn_bits = 3 + 14 + 3 * (uint32_t)hclen + rle_extra + (uint32_t)dl * nmatch;
        for (int s = 0; s < NLIT; ++s) {
            const uint32_t k = sh.hist[s];
            extra += k * (uint32_t)symbol_extra_bits(s);
            fixed_bits += k * (uint32_t)fixed_length(s);
            dyn_bits += k * ll[s];
        }
        for (int s = 0; s < NCL; ++s) dyn_bits += sh.clhist[s] * sh.cl[s];
        fixed_bits += extra;
        dyn_bits += extra;
        const uint32_t stored_bits = 40 + 8 * (uint32_t)n;
        int btype = 0;
        uint32_t best = stored_bits;
        if (fixed_bits < best) {
            btype = 1;
            best = fixed_bits;
        }
        if (dyn_bits < best) btype = 2;
        sh.btype = btype;
        if (btype != 0) {
            BitWriter bw(out32 + 2, 0);
            bw.put((uint32_t)btype << 1, 3);
            if (btype == 2) {
                uint16_t clc[NCL];
                canonical_codes(sh.cl, NCL, clc);
                bw.put((uint32_t)(hlit - 257), 5);
                bw.put(0, 5);
                bw.put((uint32_t)(hclen - 4), 4);
                for (int i = 0; i < hclen; ++i) bw.put(sh.cl[order[i]], 3);
                rle_lengths(sh.seq, hlit + 1, [&](int s, int ev, int eb) {
                    bw.put(clc[s], sh.cl[s]);
                    if (eb) bw.put((uint32_t)ev, eb);
                });
                sh.dist_bits = dl;
            } else {
                for (int s = 0; s < MAX_SYMS; ++s) ll[s] = (uint8_t)fixed_length(s);
                sh.dist_bits = 5;
            }
            canonical_codes(ll, MAX_SYMS, sh.codes);
            sh.header_bits = bw.word * 32 + (uint32_t)bw.n;
            bw.finish();
        }
    }
    __syncthreads();

    uint32_t payload;                                  // bytes of the IDAT's data
    if (sh.btype == 0) {
        if (tid == 0) {
            out8[8] = 0;
            out8[9] = (uint8_t)n;
            out8[10] = (uint8_t)(n >> 8);
            out8[11] = (uint8_t)~n;
            out8[12] = (uint8_t)(~n >> 8);
            out8[13 + n] = final_chunk ? 1 : 0;
            out8[13 + n + 3] = 0xFF;
            out8[13 + n + 4] = 0xFF;
        }
        for (int i = tid; i < n; i += THREADS) out8[13 + i] = (uint8_t)at(data, i);
        payload = (uint32_t)n + 10;
    } else {
        const int dist_bits = sh.dist_bits;
        uint32_t mine = 0;
        walk(data, seg0, seg1, s0, after, [&](int sym, int, int eb, bool m) { mine += (uint32_t)sh.lens[sym] + (uint32_t)eb + (m ? (uint32_t)dist_bits : 0u); });
        int sc = 0;
        sh.scan[0][tid] = mine;
        __syncthreads();
        for (int d = 1; d < THREADS; d <<= 1) {
            const uint32_t x = sh.scan[sc][tid] + (tid >= d ? sh.scan[sc][tid - d] : 0);
            sh.scan[sc ^ 1][tid] = x;
            sc ^= 1;
            __syncthreads();
        }
        const uint32_t pos = sh.header_bits + sh.scan[sc][tid] - mine;
        BitWriter bw(out32 + 2, pos);
        walk(data, seg0, seg1, s0, after, [&](int sym, int ev, int eb, bool m) {
            const int l = sh.lens[sym];
            bw.put((uint32_t)sh.codes[sym] | ((uint32_t)ev << l), l + eb + (m ? dist_bits : 0));      // the distance code of 1 is all zero bits
        });
        bw.finish();
        const uint32_t end = sh.header_bits + sh.scan[sc][THREADS - 1] + sh.lens[256];                 // behind the end-of-block code
        const uint32_t sync_at = (end + 3 + 7) >> 3;                                                   // byte of 00 00 FF FF
        __syncthreads();
        if (tid == 0) {
            BitWriter eob(out32 + 2, end - sh.lens[256]);
            eob.put(sh.codes[256], sh.lens[256]);
            eob.put(final_chunk ? 1u : 0u, 3);
            eob.finish();
            out8[8 + sync_at + 2] = 0xFF;
            out8[8 + sync_at + 3] = 0xFF;
        }
        payload = sync_at + 4;
    }
    if (tid == 0) {
        out8[0] = (uint8_t)(payload >> 24);
        out8[1] = (uint8_t)(payload >> 16);
        out8[2] = (uint8_t)(payload >> 8);
        out8[3] = (uint8_t)payload;
        out8[4] = 'I';
        out8[5] = 'D';
        out8[6] = 'A';
        out8[7] = 'T';
    }
    __syncthreads();

    // CRC-32 of type + data: the message (its first four bytes inverted, which is the CRC's preset) in pieces aligned to its END, so
    // that every piece but the first is whole; a piece's remainder, then a tree of  left * x^(8 |right|) + right  mod P
    {
        const int L = 4 + (int)payload;
        const int lo = L - (THREADS - tid) * CRC_PIECE;
        uint32_t r = 0;
        for (int i = max(lo, 0); i < lo + CRC_PIECE; ++i) {
            const uint32_t b = (uint32_t)out8[4 + i] ^ (i < 4 ? 255u : 0u);
            r = sh.crc_table[(r ^ b) & 255] ^ (r >> 8);
        }
        sh.crc[tid] = r;
        __syncthreads();
        for (int l = 0; l < 8; ++l) {
            const int step = 1 << l;
            if ((tid & (2 * step - 1)) == 0) sh.crc[tid] = mulmod(sh.crc[tid], CRC_SHIFT.x[l]) ^ sh.crc[tid + step];
            __syncthreads();
        }
        if (tid == 0) {
            const uint32_t crc = ~sh.crc[0];
            out8[8 + payload] = (uint8_t)(crc >> 24);
            out8[9 + payload] = (uint8_t)(crc >> 16);
            out8[10 + payload] = (uint8_t)(crc >> 8);
            out8[11 + payload] = (uint8_t)crc;
            a.size[c] = 12 + (uint64_t)payload;
            a.adler[c] = (uint64_t)(sh.s1 % 65521ull) | ((uint64_t)(sh.s2 % 65521ull) << 32);
        }
        __syncthreads();
    }
    uint4* to = reinterpret_cast<uint4*>(a.slot + c * SLOT);
    const uint4* image = reinterpret_cast<const uint4*>(out8);
    for (int i = tid; i * 16 < 12 + (int)payload; i += THREADS) to[i] = image[i];
}

// Exclusive scan of size[0 .. n) into offs by one workgroup of 1024 with a carry; *total_out = the sum.
__global__ __launch_bounds__(1024) void png_scan64(const uint64_t* size, uint64_t* offs, int64_t n, uint64_t* total_out) {
    __shared__ uint64_t buf[2][1024];
    const uint64_t total = codec::group_scan_1024<uint64_t>(n, buf, [&](int64_t i) { return size[i]; }, [&](int64_t i, uint64_t x) { offs[i] = x; });
    if (threadIdx.x == 0) *total_out = total;
}

// slot c -> out[HEAD_BYTES + offs[c] ..): bytes up to the first dword boundary of `out`, dwords assembled from two of the slot's, bytes
__global__ __launch_bounds__(THREADS) void png_gather(const uint8_t* slot, const uint64_t* size, const uint64_t* offs, uint8_t* out, uint64_t out_cap) {
    const int64_t c = blockIdx.x;
    const int sz = (int)size[c];
    const uint64_t base = HEAD_BYTES + offs[c];
    const uint8_t* src = slot + c * SLOT;
    const uint32_t* src32 = reinterpret_cast<const uint32_t*>(src);
    const int head = min(sz, (int)((4 - ((reinterpret_cast<uintptr_t>(out) + base) & 3)) & 3));
    const int words = (sz - head) >> 2;
    const int tail0 = head + 4 * words;
    const int tid = threadIdx.x;
    if (tid < head && base + tid < out_cap) out[base + tid] = src[tid];
    if (tid < sz - tail0 && base + tail0 + tid < out_cap) out[base + tail0 + tid] = src[tail0 + tid];
    const int sh = head * 8;
    for (int k = tid; k < words; k += THREADS) {
        const uint64_t o = base + head + 4 * (uint64_t)k;
        const uint32_t w0 = src32[k], w1 = src32[k + 1];         // k + 1 stays inside the slot: 4 (words + 1) <= sz + 4 <= SLOT
        const uint32_t v = sh ? (w0 >> sh) | (w1 << (32 - sh)) : w0;
        if (o + 4 <= out_cap) {
            *reinterpret_cast<uint32_t*>(out + o) = v;
        } else {
            for (int j = 0; j < 4; ++j)
                if (o + j < out_cap) out[o + j] = (uint8_t)(v >> (8 * j));
        }
    }
}

__global__ __launch_bounds__(THREADS) void png_finish(const Head h, const uint64_t* adler, int64_t nchunks, int64_t N, const uint64_t* meta, uint8_t* out,
                                                      uint64_t out_cap, uint64_t* out_len) {
    __shared__ uint8_t tail[TAIL_BYTES];
    const int tid = threadIdx.x;
    if (tid < HEAD_BYTES && (uint64_t)tid < out_cap) out[tid] = h.bytes[tid];
    // the stream's Adler-32 from the chunks' sums, then the tail by lane 0
    codec::adler_fold<CHUNK, THREADS>(adler, nchunks, N, [&](uint32_t ad) {
        const uint8_t t[TAIL_BYTES] = {0, 0, 0, 4, 'I', 'D', 'A', 'T', (uint8_t)(ad >> 24), (uint8_t)(ad >> 16), (uint8_t)(ad >> 8), (uint8_t)ad, 0, 0, 0, 0,
                                       0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
        for (int i = 0; i < TAIL_BYTES; ++i) tail[i] = t[i];
        const uint32_t crc = crc_bytes(tail + 4, 8);
        tail[12] = (uint8_t)(crc >> 24);
        tail[13] = (uint8_t)(crc >> 16);
        tail[14] = (uint8_t)(crc >> 8);
        tail[15] = (uint8_t)crc;
    });
    __syncthreads();
    const uint64_t end = HEAD_BYTES + meta[0];
    if (tid < TAIL_BYTES && end + tid < out_cap) out[end + tid] = tail[tid];
    if (tid == 0) {
        out_len[0] = end + TAIL_BYTES;
        out_len[1] = end + TAIL_BYTES > out_cap ? 1 : 0;
    }
}

}  // namespace

hipError_t launch_encode(const Plan& p, const EncodeArgs& a, const Head& h, hipStream_t s) {
    static unsigned long long lds_set = 0;
    hipError_t e = hipSuccess;
    {
        int dev = 0;
        if ((e = hipGetDevice(&dev)) != hipSuccess) return e;
        if (dev >= 64 || !((lds_set >> dev) & 1ull)) {      // more than 64 KiB of dynamic LDS: an opt-in per device
            if ((e = hipFuncSetAttribute(reinterpret_cast<const void*>(png_chunk), hipFuncAttributeMaxDynamicSharedMemorySize, (int)CHUNK_LDS)) != hipSuccess) return e;
            if (dev < 64) lds_set |= 1ull << dev;
        }
    }
    FilterArgs f{a.src, a.src_stride, p.W, p.C, p.depth / 8, a.flip && p.C >= 3, p.row, a.filt};
    hipLaunchKernelGGL(png_filter, dim3((unsigned)p.H), dim3(THREADS), 0, s, f);
    ChunkArgs c{a.filt, p.N, p.nchunks, a.slot, a.size, a.adler};
    hipLaunchKernelGGL(png_chunk, dim3((unsigned)p.nchunks), dim3(THREADS), CHUNK_LDS, s, c);
    hipLaunchKernelGGL(png_scan64, dim3(1), dim3(1024), 0, s, a.size, a.offs, p.nchunks, a.meta);
    hipLaunchKernelGGL(png_gather, dim3((unsigned)p.nchunks), dim3(THREADS), 0, s, a.slot, a.size, a.offs, a.out, a.out_cap);
    hipLaunchKernelGGL(png_finish, dim3(1), dim3(THREADS), 0, s, h, a.adler, p.nchunks, p.N, a.meta, a.out, a.out_cap, a.out_len);
    return hipGetLastError();
}

}  // namespace png
}  // namespace nesr

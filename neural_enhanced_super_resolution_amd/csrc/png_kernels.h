// Launcher of the PNG encoder (png.hip), the layout of its scratch, and the serial pieces of the deflate coder that the host and the
// device share: code-length construction, canonical codes, run coding of the lengths (tests/png_ref.py is the specification).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define NESR_PNG_HD __host__ __device__ inline

namespace nesr {
namespace png {

constexpr int CHUNK = 32768;               // S: filtered bytes per deflate chunk = per IDAT
constexpr int HEAD_BYTES = 47;             // signature 8, IHDR 25, IDAT[78 01] 14
constexpr int TAIL_BYTES = 28;             // IDAT[Adler-32] 16, IEND 12
constexpr int CHUNK_OVERHEAD = 22;         // of a stored chunk: IDAT framing 12, block header 5, sync 5
constexpr int SLOT = 32800;                // bytes of one chunk's IDAT in the scratch: CHUNK + CHUNK_OVERHEAD, rounded up to 16
constexpr int NLIT = 286, NCL = 19;
constexpr int MAX_SYMS = 288;

struct Head {
    uint8_t bytes[HEAD_BYTES + 1];
};

// Regions of the scratch, each 256-byte aligned (png_api.cpp: plan())
struct Plan {
    int H, W, C, depth, bpp;
    int64_t row;                           // 1 + W * bpp: bytes of a filtered row
    int64_t N;                             // H * row: bytes of the filtered stream
    int64_t nchunks;                       // ceil(N / CHUNK)
    size_t off_filt, off_slot, off_size, off_offs, off_adler, off_meta, total;
};

struct EncodeArgs {
    const uint8_t* src;
    int64_t src_stride;
    int flip;                              // the frame is B G R (A): channels 0 and 2 swap on the way into the file
    uint8_t* filt;                         // [N] the filtered stream
    uint8_t* slot;                         // [nchunks][SLOT] each chunk's IDAT, framing and CRC included
    uint64_t* size;                        // [nchunks] bytes of each IDAT
    uint64_t* offs;                        // [nchunks] their exclusive scan
    uint64_t* adler;                       // [nchunks] (sum of bytes mod 65521) | (weighted sum mod 65521) << 32
    uint64_t* meta;                        // [0] bytes of all data IDATs
    uint8_t* out;
    uint64_t out_cap;
    uint64_t* out_len;                     // [0] bytes of the file  [1] 1 if it did not fit
};

hipError_t launch_encode(const Plan& p, const EncodeArgs& a, const Head& h, hipStream_t s);

// ---------------------------------------------------------------------------------------------------------------- shared serial pieces
struct HuffWork {
    uint32_t iw[NLIT];                     // weights of the internal nodes, in creation order
    uint16_t order[NLIT];                  // used symbols, ascending by (count, symbol)
    uint16_t pl[NLIT], pi[NLIT], di[NLIT]; // parent of leaf / of internal node; depth of internal node
    uint16_t bl[16];                       // codes per length
};

// used symbols sorted ascending by (count, symbol) into w.order -> their number.  (The device ranks them in parallel instead.)
NESR_PNG_HD int sort_used(const uint32_t* counts, int n, HuffWork& w) {
    int m = 0;
    for (int s = 0; s < n; ++s) {
        if (!counts[s]) continue;
        int j = m++;
        while (j > 0 && counts[w.order[j - 1]] > counts[s]) {     // equal counts keep the symbol order: s rises
            w.order[j] = w.order[j - 1];
            --j;
        }
        w.order[j] = (uint16_t)s;
    }
    return m;
}

// png_ref.code_lengths with the sort done: w.order[0 .. m) holds the used symbols.  The sum of the counts must stay below 2^32.
NESR_PNG_HD void code_lengths_sorted(const uint32_t* counts, int m, int n, int limit, uint8_t* lengths, HuffWork& w) {
    for (int i = 0; i < n; ++i) lengths[i] = 0;
    if (m < 2) {
        const int s = m ? w.order[0] : 0;
        lengths[s] = 1;
        lengths[s == 0 ? 1 : 0] = 1;
        return;
    }
    int li = 0, ii = 0;
    for (int k = 0; k < m - 1; ++k) {
        uint32_t tot = 0;
        for (int t = 0; t < 2; ++t) {
            if (li < m && (ii >= k || counts[w.order[li]] <= w.iw[ii])) {      // a leaf before an internal node of equal weight
                tot += counts[w.order[li]];
                w.pl[li++] = (uint16_t)k;
            } else {
                tot += w.iw[ii];
                w.pi[ii++] = (uint16_t)k;
            }
        }
        w.iw[k] = tot;
    }
    w.di[m - 2] = 0;
    for (int k = m - 3; k >= 0; --k) w.di[k] = (uint16_t)(w.di[w.pi[k]] + 1);
    for (int d = 0; d < 16; ++d) w.bl[d] = 0;
    for (int i = 0; i < m; ++i) {
        const int d = w.di[w.pl[i]] + 1;
        ++w.bl[d > limit ? limit : d];
    }
    uint32_t total = 0;
    for (int d = 1; d <= limit; ++d) total += (uint32_t)w.bl[d] << (limit - d);
    while (total > (1u << limit)) {                                           // the repair rule
        --w.bl[limit];
        for (int d = limit - 1; d > 0; --d) {
            if (w.bl[d]) {
                --w.bl[d];
                w.bl[d + 1] += 2;
                break;
            }
        }
        --total;
    }
    int j = m;
    for (int d = 1; d <= limit; ++d)
        for (int c = 0; c < w.bl[d]; ++c) lengths[w.order[--j]] = (uint8_t)d;
}

// canonical codes (RFC 1951 3.2.2), bit-reversed: ready to be written LSB first
NESR_PNG_HD void canonical_codes(const uint8_t* lengths, int n, uint16_t* codes) {
    uint16_t bl[17] = {0}, next[17] = {0};
    for (int s = 0; s < n; ++s) ++bl[lengths[s]];
    bl[0] = 0;
    uint32_t code = 0;
    for (int d = 1; d <= 15; ++d) {
        code = (code + bl[d - 1]) << 1;
        next[d] = (uint16_t)code;
    }
    for (int s = 0; s < n; ++s) {
        const int l = lengths[s];
        codes[s] = l ? (uint16_t)(__builtin_bitreverse32((uint32_t)next[l]++) >> (32 - l)) : (uint16_t)0;
    }
}

// png_ref.rle_lengths: greedy 16 / 17 / 18 coding; sink(symbol, extra value, extra bits)
template <typename Sink>
NESR_PNG_HD void rle_lengths(const uint8_t* seq, int n, Sink&& sink) {
    int i = 0;
    while (i < n) {
        const int v = seq[i];
        int r = 1;
        while (i + r < n && seq[i + r] == v) ++r;
        if (v == 0 && r >= 3) {
            const int t = r < 138 ? r : 138;
            if (t >= 11) sink(18, t - 11, 7);
            else sink(17, t - 3, 3);
            i += t;
        } else if (v != 0 && i > 0 && seq[i - 1] == v && r >= 3) {
            const int t = r < 6 ? r : 6;
            sink(16, t - 3, 2);
            i += t;
        } else {
            sink(v, 0, 0);
            ++i;
        }
    }
}

NESR_PNG_HD int fixed_length(int s) { return s < 144 ? 8 : (s < 256 ? 9 : (s < 280 ? 7 : 8)); }
NESR_PNG_HD int symbol_extra_bits(int s) { return s < 265 || s == 285 ? 0 : (s - 261) >> 2; }

// match length 3 .. 258 -> literal/length symbol, extra value, extra bits
NESR_PNG_HD void length_symbol(int length, int& sym, int& ev, int& eb) {
    const int v = length - 3;
    if (v == 255) {
        sym = 285;
        ev = eb = 0;
    } else if (v < 8) {
        sym = 257 + v;
        ev = eb = 0;
    } else {
        eb = 29 - __builtin_clz((unsigned)v);              // floor(log2 v) - 2
        sym = 261 + 4 * eb + ((v >> eb) & 3);
        ev = v & ((1 << eb) - 1);
    }
}

}  // namespace png
}  // namespace nesr

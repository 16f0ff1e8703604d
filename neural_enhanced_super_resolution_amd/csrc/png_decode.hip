// PNG decoder kernels for gfx950 (tests/png_decode_ref.py is the specification; the status bits are those of png_decode_kernels.h).
//
//   pngd_inflate<false>  measure: one wave per segment walks the deflate symbols and counts the bytes they give; status bits per segment
//   pngd_scan            64-bit exclusive scan of the sizes; the total must be N; writes the status word (so nothing has to clear it)
//   pngd_inflate<true>   write: the same walk, storing the filtered stream at the segment's offset
//   pngd_adler / pngd_adler_check   partial sums per 32 KiB piece, folded as the encoder's finish pass folds them
//   pngd_unfilter        the five row filters undone, the channel flip, the big-endian swap and the strided store in one pass
//
// Rules.  No workgroup waits on another: order between the passes is the launch order on the stream.  Every turn of a decode loop
// consumes at least one bit or ends the segment, and the bit reader reports TRUNC once more bits are consumed than the segment holds.
// Every store into the stream is guarded by N, every store into the frame by H, W; a segment is read only after offset + bytes <= n was
// checked.  A pass that finds a non-zero status word does nothing, so a corrupt or dependent file ends in that word and never in a fault.
//
// The inflate wave.  Lane 0 walks the symbols (a 10-bit look-up table per code in LDS, built by all lanes per dynamic block and once
// per wave for the fixed code; longer codes bit by bit); literals go straight into a 32 KiB window in LDS.  A match is copied by all lanes inside that window -- the source lies wholly
// before the destination, so lane i takes byte (i mod distance) of the source and an overlapped copy repeats -- and the window is
// flushed to the stream by all lanes.  Matches therefore never read back what the wave stored to global memory: LDS operations of one
// wave execute in order, and the barrier between lane 0's turn and the copy is a workgroup barrier of one wave.
#include "codec_device.h"
#include "png_decode_kernels.h"

namespace nesr {
namespace pngdec {
namespace {

constexpr int FAST = 10;
constexpr int WINDOW = 32768;
constexpr int FLUSH_AT = 8192;
constexpr int WAVE = 64;

__device__ const uint16_t LEN_BASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__device__ const uint8_t LEN_EXTRA[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__device__ const uint16_t DIST_BASE[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
__device__ const uint8_t DIST_EXTRA[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
__device__ const uint8_t CL_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

enum { ACT_NONE = 0, ACT_TABLES, ACT_MATCH, ACT_STORED, ACT_FLUSH, ACT_DONE };
enum { MODE_HEADER = 0, MODE_HUFF, MODE_AFTER };

struct Code {
    uint16_t count[16];                    // codes per length
    uint16_t sym[288];                     // symbols sorted by (length, symbol)
    uint16_t fast[1 << FAST];              // next FAST bits -> symbol << 4 | length; 0: a longer code or none
};

struct Shared {
    Code lit, dist, cl;
    Code flit, fdist;                      // the fixed code's pair, built by the first BTYPE 1 block of the wave and kept
    uint8_t lens[320];                     // the lengths of the block's two codes, one sequence
    uint16_t code[320];                    // their canonical codes
    int action, hlit, hdist, len, dist_v, fixed;
    int64_t src, pos, pos_end;
};

// LSB-first bit reader over src[0 .. nbytes); past the end it feeds zeros and `over()` turns true
struct Bits {
    const uint8_t* src;
    int64_t nbytes, next, consumed, total;
    uint64_t buf;
    int cnt;

    __device__ void init(const uint8_t* s, int64_t n) {
        src = s;
        nbytes = n;
        next = 0;
        consumed = 0;
        total = 8 * n;
        buf = 0;
        cnt = 0;
    }
    __device__ uint32_t peek(int n) {
        while (cnt <= 56) {
            const uint64_t b = next < nbytes ? src[next] : 0;
            buf |= b << cnt;
            cnt += 8;
            ++next;
        }
        return (uint32_t)(buf & ((1ull << n) - 1));
    }
    __device__ void drop(int n) {
        buf >>= n;
        cnt -= n;
        consumed += n;
    }
    __device__ uint32_t take(int n) {
        const uint32_t v = peek(n);
        drop(n);
        return v;
    }
    __device__ bool over() const { return consumed > total; }
    __device__ void seek_byte(int64_t byte) {
        consumed = 8 * byte;
        next = byte;
        buf = 0;
        cnt = 0;
    }
};

// lens[0 .. n) -> count, sym and the canonical codes; -> left (0 complete, > 0 incomplete, < 0 over-subscribed: nothing else is valid then)
__device__ int build_code(const uint8_t* lens, int n, Code& c, uint16_t* code) {
    for (int d = 0; d < 16; ++d) c.count[d] = 0;
    for (int s = 0; s < n; ++s) ++c.count[lens[s]];
    int left = 1;
    for (int d = 1; d < 16; ++d) {
        left = (left << 1) - c.count[d];
        if (left < 0) return left;
    }
    uint32_t offs[16], next[16];           // indexed by constants after unrolling; small either way
    offs[1] = 0;
    next[0] = 0;
    uint32_t cd = 0;
    uint16_t prev = 0;
    for (int d = 1; d < 16; ++d) {
        if (d > 1) offs[d] = offs[d - 1] + c.count[d - 1];
        cd = (cd + prev) << 1;
        next[d] = cd;
        prev = c.count[d];
    }
    for (int s = 0; s < n; ++s) {
        const int l = lens[s];
        if (!l) continue;
        c.sym[offs[l]++] = (uint16_t)s;
        code[s] = (uint16_t)next[l]++;
    }
    return left;
}

// all lanes: the look-up table of a code from lens / code
__device__ void fill_fast(const uint8_t* lens, const uint16_t* code, int n, Code& c, int lane) {
    for (int s = lane; s < n; s += WAVE) {
        const int l = lens[s];
        if (l == 0 || l > FAST) continue;
        const uint32_t r = __builtin_bitreverse32((uint32_t)code[s]) >> (32 - l);
        for (uint32_t k = r; k < (1u << FAST); k += 1u << l) c.fast[k] = (uint16_t)((s << 4) | l);
    }
}

// one symbol, bit by bit (puff's loop); -1 with *st set: TRUNC or BADCODE
__device__ int decode_slow(Bits& r, const Code& c, uint32_t* st) {
    int code = 0, first = 0, index = 0;
    for (int d = 1; d < 16; ++d) {
        code |= (int)r.take(1);
        if (r.over()) {
            *st |= ST_TRUNC;
            return -1;
        }
        const int cnt = c.count[d];
        if (code - cnt < first) return c.sym[index + code - first];
        index += cnt;
        first = (first + cnt) << 1;
        code <<= 1;
    }
    *st |= ST_BADCODE;
    return -1;
}

__device__ int decode_sym(Bits& r, const Code& c, uint32_t* st) {
    const uint32_t e = c.fast[r.peek(FAST)];
    if (e) {
        r.drop((int)(e & 15));
        if (r.over()) {
            *st |= ST_TRUNC;
            return -1;
        }
        return (int)(e >> 4);
    }
    return decode_slow(r, c, st);
}

// lane 0: BTYPE 1 or 2 -> sh.lens, sh.hlit, sh.hdist and the sorted forms of both codes (sh.flit / sh.fdist for BTYPE 1, once per
// wave: `fixed_ready`); *fill: the look-up tables are still to be filled from them; false with *st set on a broken header
__device__ bool block_codes(Bits& r, int btype, Shared& sh, bool& fixed_ready, bool* fill, uint32_t* st) {
    *fill = true;
    if (btype == 1) {
        if (fixed_ready) return *fill = false, true;
        fixed_ready = true;
        for (int s = 0; s < 288; ++s) sh.lens[s] = (uint8_t)(s < 144 ? 8 : (s < 256 ? 9 : (s < 280 ? 7 : 8)));
        for (int s = 288; s < 320; ++s) sh.lens[s] = 5;
        sh.hlit = 288;
        sh.hdist = 32;
    } else {
        const int hlit = (int)r.take(5) + 257, hdist = (int)r.take(5) + 1, hclen = (int)r.take(4) + 4;
        if (r.over()) return *st |= ST_TRUNC, false;
        if (hlit > 286 || hdist > 30) return *st |= ST_BADHEADER, false;
        uint8_t* cl = sh.lens + 300;       // 19 bytes at the far end; read before the sequence can reach them (it is checked below)
        for (int i = 0; i < 19; ++i) cl[i] = 0;
        for (int i = 0; i < hclen; ++i) cl[CL_ORDER[i]] = (uint8_t)r.take(3);
        if (r.over()) return *st |= ST_TRUNC, false;
        if (build_code(cl, 19, sh.cl, sh.code) != 0) return *st |= ST_BADHEADER, false;
        // the sequence may grow to 316 entries and would then overwrite cl: keep the code-length code's sorted form only (sh.cl)
        const int n = hlit + hdist;
        int at = 0;
        while (at < n) {
            const int s = decode_slow(r, sh.cl, st);
            if (s < 0) return false;
            if (s < 16) {
                sh.lens[at++] = (uint8_t)s;
                continue;
            }
            int v = 0, rep;
            if (s == 16) {
                if (at == 0) return *st |= ST_BADHEADER, false;
                v = sh.lens[at - 1];
                rep = 3 + (int)r.take(2);
            } else if (s == 17) {
                rep = 3 + (int)r.take(3);
            } else {
                rep = 11 + (int)r.take(7);
            }
            if (r.over()) return *st |= ST_TRUNC, false;
            if (at + rep > n) return *st |= ST_BADHEADER, false;
            for (int k = 0; k < rep; ++k) sh.lens[at++] = (uint8_t)v;
        }
        if (sh.lens[256] == 0) return *st |= ST_BADHEADER, false;
        sh.hlit = hlit;
        sh.hdist = hdist;
    }
    Code& lit = btype == 1 ? sh.flit : sh.lit;
    Code& dist = btype == 1 ? sh.fdist : sh.dist;
    const int left_l = build_code(sh.lens, sh.hlit, lit, sh.code);
    int nlit = 0;
    for (int d = 1; d < 16; ++d) nlit += lit.count[d];
    if (left_l != 0 && !(left_l > 0 && nlit == 1 && lit.count[1] == 1)) return *st |= ST_BADHEADER, false;
    const int left_d = build_code(sh.lens + sh.hlit, sh.hdist, dist, sh.code + sh.hlit);
    if (left_d < 0) return *st |= ST_BADHEADER, false;
    int ndist = 0;
    for (int d = 1; d < 16; ++d) ndist += dist.count[d];
    if (left_d > 0 && ndist > 0 && !(ndist == 1 && dist.count[1] == 1)) return *st |= ST_BADHEADER, false;
    return true;
}

template <bool WRITE>
__global__ __launch_bounds__(WAVE) void pngd_inflate(const InflateArgs a) {
    __shared__ Shared sh;
    __shared__ uint8_t win[WRITE ? WINDOW : 16];
    const int lane = threadIdx.x;
    const int64_t seg = blockIdx.x;
    if (WRITE && *a.status != 0) return;
    const nesr_png_segment sg = a.segs[seg];
    uint32_t st = 0;
    const bool inside = sg.offset >= 0 && sg.bytes >= 1 && (uint64_t)sg.offset <= a.n && (uint64_t)sg.bytes <= a.n - (uint64_t)sg.offset;
    if (!inside) {
        if (lane == 0) {
            if (WRITE) {
                atomicOr(a.status, ST_TRUNC);
            } else {
                a.size[seg] = 0;
                a.segst[seg] = ST_TRUNC;
            }
        }
        return;
    }
    const uint8_t* src = a.file + sg.offset;
    const int64_t base = WRITE ? (int64_t)a.offs[seg] : 0;
    const int64_t cap = WRITE ? a.N - base : a.N;       // bytes this segment may still give
    const bool last = sg.last != 0;
    Bits r;
    r.init(src, sg.bytes);
    int mode = MODE_HEADER, final_block = 0;
    bool fixed_ready = false, fill = false;                // lane 0's
    const Code* lit = &sh.lit;
    const Code* dist = &sh.dist;
    int64_t pos = 0, flushed = 0;

    for (;;) {
        if (lane == 0) {
            int action = ACT_NONE;
            while (action == ACT_NONE) {
                if (mode == MODE_AFTER) {
                    if (final_block) {
                        if (!last || ((r.consumed + 7) >> 3) != r.nbytes) st |= ST_BADEND;
                        action = ACT_DONE;
                        break;
                    }
                    mode = MODE_HEADER;
                }
                if (mode == MODE_HEADER) {
                    if (!last && r.consumed == r.total && r.consumed > 0) {
                        action = ACT_DONE;
                        break;
                    }
                    final_block = (int)r.take(1);
                    const int btype = (int)r.take(2);
                    if (r.over()) {
                        st |= ST_TRUNC;
                    } else if (btype == 3) {
                        st |= ST_BADHEADER;
                    } else if (btype == 0) {
                        r.drop((int)((-r.consumed) & 7));
                        const uint32_t ln = r.take(16), nl = r.take(16);
                        const int64_t p = r.consumed >> 3;
                        if (r.over()) {
                            st |= ST_TRUNC;
                        } else if (ln != (~nl & 0xFFFFu)) {
                            st |= ST_BADSTORED;
                        } else if (p + (int64_t)ln > r.nbytes) {
                            st |= ST_TRUNC;
                        } else if (pos + (int64_t)ln > cap) {
                            st |= ST_TOTAL;
                        } else {
                            sh.src = p;
                            sh.len = (int)ln;
                            sh.pos = pos;
                            pos += ln;
                            r.seek_byte(p + ln);
                            mode = MODE_AFTER;
                            action = WRITE ? ACT_STORED : ACT_NONE;
                        }
                    } else if (block_codes(r, btype, sh, fixed_ready, &fill, &st)) {
                        mode = MODE_HUFF;
                        lit = btype == 1 ? &sh.flit : &sh.lit;
                        dist = btype == 1 ? &sh.fdist : &sh.dist;
                        sh.fixed = btype == 1;
                        action = fill ? ACT_TABLES : ACT_NONE;
                    }
                    if (st) action = ACT_DONE;
                    continue;
                }
                // MODE_HUFF
                const int s = decode_sym(r, *lit, &st);
                if (s < 0) {
                    action = ACT_DONE;
                } else if (s < 256) {
                    if (pos + 1 > cap) {
                        st |= ST_TOTAL;
                        action = ACT_DONE;
                    } else {
                        if (WRITE) win[(uint32_t)pos & (WINDOW - 1)] = (uint8_t)s;
                        ++pos;
                        if (WRITE && pos - flushed >= FLUSH_AT) action = ACT_FLUSH;
                    }
                } else if (s == 256) {
                    mode = MODE_AFTER;
                } else if (s > 285) {
                    st |= ST_BADCODE;
                    action = ACT_DONE;
                } else {
                    const int ln = LEN_BASE[s - 257] + (int)r.take(LEN_EXTRA[s - 257]);
                    if (r.over()) {
                        st |= ST_TRUNC;
                        action = ACT_DONE;
                        break;
                    }
                    const int d = decode_sym(r, *dist, &st);
                    if (d < 0) {
                        action = ACT_DONE;
                        break;
                    }
                    if (d > 29) {
                        st |= ST_BADCODE;
                        action = ACT_DONE;
                        break;
                    }
                    const int dist = DIST_BASE[d] + (int)r.take(DIST_EXTRA[d]);
                    if (r.over()) {
                        st |= ST_TRUNC;
                    } else if ((int64_t)dist > pos) {
                        st |= ST_DEPENDENT;
                    } else if (pos + ln > cap) {
                        st |= ST_TOTAL;
                    } else {
                        sh.len = ln;
                        sh.dist_v = dist;
                        sh.pos = pos;
                        pos += ln;
                        action = WRITE ? ACT_MATCH : ACT_NONE;
                    }
                    if (st) action = ACT_DONE;
                }
            }
            sh.action = action;
            sh.pos_end = pos;
        }
        __syncthreads();
        const int action = sh.action;
        const int64_t pos_end = sh.pos_end;
        if (action == ACT_TABLES) {
            Code& tl = sh.fixed ? sh.flit : sh.lit;
            Code& td = sh.fixed ? sh.fdist : sh.dist;
            for (int k = lane; k < (1 << FAST); k += WAVE) tl.fast[k] = td.fast[k] = 0;
            __syncthreads();
            fill_fast(sh.lens, sh.code, sh.hlit, tl, lane);
            fill_fast(sh.lens + sh.hlit, sh.code + sh.hlit, sh.hdist, td, lane);
        } else if (WRITE && action == ACT_MATCH) {
            const int len = sh.len, dist = sh.dist_v;
            const uint32_t p = (uint32_t)sh.pos;
            for (int i = lane; i < len; i += WAVE) {             // ascending i: a slot is read no later than it is written
                const int j = dist >= len ? i : i % dist;
                const uint8_t v = win[(p - (uint32_t)dist + (uint32_t)j) & (WINDOW - 1)];
                win[(p + (uint32_t)i) & (WINDOW - 1)] = v;
            }
        }
        if (WRITE) {
            const bool stored = action == ACT_STORED;
            const int64_t upto = stored ? sh.pos : pos_end;
            if (stored || action == ACT_DONE || upto - flushed >= FLUSH_AT) {
                __syncthreads();
                for (int64_t i = flushed + lane; i < upto; i += WAVE)
                    if (base + i < a.N) a.filt[base + i] = win[(uint32_t)i & (WINDOW - 1)];
                flushed = upto;
            }
            if (stored) {
                __syncthreads();
                const int64_t p = sh.src;
                const int len = sh.len;
                for (int i = lane; i < len; i += WAVE) {         // a lane's slots recur in its own later turns: the last byte wins
                    const uint8_t v = src[p + i];
                    win[(uint32_t)(upto + i) & (WINDOW - 1)] = v;
                    if (base + upto + i < a.N) a.filt[base + upto + i] = v;
                }
                flushed = upto + len;
            }
        }
        __syncthreads();
        if (action == ACT_DONE) break;
    }
    if (lane == 0) {
        if (WRITE) {
            if (st) atomicOr(a.status, st);
        } else {
            a.size[seg] = (uint64_t)pos;
            a.segst[seg] = st;
        }
    }
}

// Exclusive scan of size[0 .. n) into offs by one workgroup of 1024 with a carry; the status word = the OR of the segments' bits, and
// TOTAL when they are clean and the sum is not N.
__global__ __launch_bounds__(1024) void pngd_scan(const uint64_t* size, const uint32_t* segst, uint64_t* offs, int64_t n, int64_t N, uint32_t* status) {
    __shared__ uint64_t buf[2][1024];
    __shared__ uint32_t bits;
    const int tid = threadIdx.x;
    if (tid == 0) bits = 0;
    uint32_t mine = 0;
    const uint64_t total = codec::group_scan_1024<uint64_t>(
        n, buf,
        [&](int64_t i) {
            mine |= segst[i];
            return size[i];
        },
        [&](int64_t i, uint64_t x) { offs[i] = x; });
    if (mine) atomicOr(&bits, mine);
    __syncthreads();
    if (tid == 0) *status = bits ? bits : (total != (uint64_t)N ? ST_TOTAL : 0u);
}

__global__ void pngd_clear(uint32_t* status) { *status = 0; }

// (sum of bytes mod 65521) | (sum of (n - i) b[i] mod 65521) << 32 of one piece of n <= ADLER_PIECE bytes
__global__ __launch_bounds__(256) void pngd_adler(const uint8_t* filt, int64_t N, uint64_t* adler, const uint32_t* status) {
    __shared__ unsigned long long s1, s2;
    if (*status != 0) return;
    const int tid = threadIdx.x;
    if (tid == 0) s1 = s2 = 0;
    __syncthreads();
    const int64_t at = (int64_t)blockIdx.x * ADLER_PIECE;
    const int n = (int)min((int64_t)ADLER_PIECE, N - at);
    constexpr int PER = ADLER_PIECE / 256;
    unsigned long long a = 0, b = 0;
    for (int k = 0; k < PER; ++k) {
        const int i = tid * PER + k;
        if (i < n) {
            const unsigned v = filt[at + i];
            a += v;
            b += (unsigned long long)(n - i) * v;
        }
    }
    atomicAdd(&s1, a);
    atomicAdd(&s2, b);
    __syncthreads();
    if (tid == 0) adler[blockIdx.x] = (uint64_t)(s1 % 65521ull) | ((uint64_t)(s2 % 65521ull) << 32);
}

// Adler-32 of the stream from the pieces' sums: a' = a + s1, b' = b + n a + s2 (mod 65521); each lane folds a run of pieces from
// (0, 0), lane 0 chains the runs.  A mismatch with the file's value sets ADLER.
__global__ __launch_bounds__(256) void pngd_adler_check(const uint64_t* adler, int64_t npieces, int64_t N, uint32_t expect, uint32_t* status) {
    if (*status != 0) return;
    codec::adler_fold<ADLER_PIECE, 256>(adler, npieces, N, [&](uint32_t got) {
        if (got != expect) atomicOr(status, ST_ADLER);
    });
}

// One workgroup per row; only the workgroup of a row that starts a group works (row 0, and rows of type 0 or 1: they need nothing from
// above).  It undoes the group's rows in bands of UNFILTER_LANES rows, one lane per row: at step t lane r holds pixel x = t - r, its
// left neighbour is its own last result, the pixel above is what lane r - 1 produced one step earlier (handed over through LDS) and the
// pixel above-left is what it handed over the step before.  The last row of a band goes to `carry` for the first lane of the next.
__device__ inline uint32_t paeth(uint32_t a, uint32_t b, uint32_t c) {
    const int p = (int)a + (int)b - (int)c;
    const int pa = abs(p - (int)a), pb = abs(p - (int)b), pc = abs(p - (int)c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__global__ __launch_bounds__(UNFILTER_LANES) void pngd_unfilter(const UnfilterArgs a) {
    __shared__ uint64_t hand[2][UNFILTER_LANES];
    __shared__ int nrows_sh;
    __shared__ uint32_t gate_sh;
    const int y0 = blockIdx.x;
    const int lane = threadIdx.x;
    // other workgroups of this launch may set FILTER in the word meanwhile: one lane reads it, so the whole workgroup decides alike
    if (lane == 0) gate_sh = *a.status;
    __syncthreads();
    if (gate_sh != 0) return;
    const uint32_t t0 = a.filt[(int64_t)y0 * a.row];
    if (t0 > 4 && lane == 0) atomicOr(a.status, ST_FILTER);
    if (y0 > 0 && t0 >= 2 && t0 <= 4) return;            // not the start of a group
    const int bpp = a.bpp;
    for (int yb = y0;; yb += UNFILTER_LANES) {
        // rows of this band: up to the next row that starts a group
        if (lane == 0) nrows_sh = min(UNFILTER_LANES, a.H - yb);
        __syncthreads();
        const int y = yb + lane;
        uint32_t type = 0;
        if (y < a.H) {
            type = a.filt[(int64_t)y * a.row];
            if (type > 4) type = 0;                        // reported by that row's own workgroup
            if (y > y0 && type < 2) atomicMin(&nrows_sh, lane);
        }
        __syncthreads();
        const int nrows = nrows_sh;
        if (nrows == 0) break;
        const bool active = lane < nrows;
        // an active lane's row is inside the frame (nrows <= H - yb): only such a lane gets pointers
        const uint8_t* in = active ? a.filt + (int64_t)y * a.row + 1 : nullptr;
        uint8_t* out = active ? a.dst + (int64_t)y * a.dst_stride : nullptr;
        const uint8_t* above = (active && lane == 0 && y > y0) ? a.carry + (int64_t)(y - 1) * (a.row - 1) : nullptr;
        uint8_t* keep = (active && lane == nrows - 1 && nrows == UNFILTER_LANES && y + 1 < a.H) ? a.carry + (int64_t)y * (a.row - 1) : nullptr;
        uint64_t left = 0, up_left = 0;
        const int steps = a.W + nrows - 1;
        for (int t = 0; t < steps; ++t) {
            const int x = t - lane;
            uint64_t res = 0;
            if (active && x >= 0 && x < a.W) {
                uint64_t up = 0;
                if (lane > 0) {
                    up = hand[(t & 1) ^ 1][lane - 1];
                } else if (above) {
                    for (int k = 0; k < bpp; ++k) up |= (uint64_t)above[(int64_t)x * bpp + k] << (8 * k);
                }
                for (int k = 0; k < bpp; ++k) {
                    const uint32_t v = in[(int64_t)x * bpp + k];
                    const uint32_t pa = (uint32_t)(left >> (8 * k)) & 255, pb = (uint32_t)(up >> (8 * k)) & 255, pc = (uint32_t)(up_left >> (8 * k)) & 255;
                    const uint32_t pred = type == 0 ? 0 : (type == 1 ? pa : (type == 2 ? pb : (type == 3 ? (pa + pb) >> 1 : paeth(pa, pb, pc))));
                    const uint32_t o = (v + pred) & 255;
                    res |= (uint64_t)o << (8 * k);
                    const int smp = k / a.bps, byt = k - smp * a.bps;
                    const int to = ((a.flip && smp < 3) ? 2 - smp : smp) * a.bps + (a.bps == 2 ? 1 - byt : 0);
                    out[(int64_t)x * bpp + to] = (uint8_t)o;
                    if (keep) keep[(int64_t)x * bpp + k] = (uint8_t)o;
                }
                left = res;
                up_left = up;
            }
            hand[t & 1][lane] = res;
            __syncthreads();
        }
        if (nrows < UNFILTER_LANES || yb + UNFILTER_LANES >= a.H) break;
        __syncthreads();                                     // `carry` of this band is visible to the workgroup's next band
    }
}

}  // namespace

hipError_t launch_inflate(const InflateArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(pngd_inflate<false>, dim3((unsigned)a.nseg), dim3(WAVE), 0, s, a);
    hipLaunchKernelGGL(pngd_scan, dim3(1), dim3(1024), 0, s, a.size, a.segst, a.offs, a.nseg, a.N, a.status);
    hipLaunchKernelGGL(pngd_inflate<true>, dim3((unsigned)a.nseg), dim3(WAVE), 0, s, a);
    hipLaunchKernelGGL(pngd_adler, dim3((unsigned)a.npieces), dim3(256), 0, s, a.filt, a.N, a.adler, a.status);
    hipLaunchKernelGGL(pngd_adler_check, dim3(1), dim3(256), 0, s, a.adler, a.npieces, a.N, a.expect_adler, a.status);
    return hipGetLastError();
}

hipError_t launch_unfilter(const UnfilterArgs& a, hipStream_t s) {
    if (a.status_gate == 0) hipLaunchKernelGGL(pngd_clear, dim3(1), dim3(1), 0, s, a.status);
    hipLaunchKernelGGL(pngd_unfilter, dim3((unsigned)a.H), dim3(UNFILTER_LANES), 0, s, a);
    return hipGetLastError();
}

}  // namespace pngdec
}  // namespace nesr

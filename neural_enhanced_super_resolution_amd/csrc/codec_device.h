// Device code the four file codecs share (jpeg.hip, jpeg_decode.hip, png.hip, png_decode.hip): the single-workgroup scan behind their
// seven scan kernels and the Adler-32 fold of per-piece sums behind png_finish and pngd_adler_check.  The kernels stay in their own
// files: each is its __shared__ buffer, one call, and what lane 0 does with the total.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nesr {
namespace codec {

// Exclusive scan of n values by one workgroup of 1024 lanes, in steps of 1024 with a carry: load(i) gives value i, store(i, x) takes
// the sum of the values before it (0 <= i < n, each called once, by lane i % 1024).  Returns the sum of all n to every lane.  The
// barrier that ends a step keeps the next step's first write to buf[0] behind this step's last read of it.
template <typename T, typename Load, typename Store>
__device__ __forceinline__ T group_scan_1024(int64_t n, T (*buf)[1024], Load&& load, Store&& store) {
    const int tid = threadIdx.x;
    T carry = 0;
    for (int64_t base = 0; base < n; base += 1024) {
        const int64_t i = base + tid;
        const T v = i < n ? load(i) : (T)0;
        int cur = 0;
        buf[0][tid] = v;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            const T x = buf[cur][tid] + (tid >= d ? buf[cur][tid - d] : (T)0);
            buf[cur ^ 1][tid] = x;
            cur ^= 1;
            __syncthreads();
        }
        const T incl = buf[cur][tid];
        const T sum = buf[cur][1023];
        if (i < n) store(i, carry + incl - v);
        carry += sum;
        __syncthreads();
    }
    return carry;
}

// Adler-32 of a stream of N bytes from the sums of its pieces of PIECE bytes (the last one shorter), sums[c] = (sum of bytes mod 65521)
// | (sum of (n - i) b[i] mod 65521) << 32:  a' = a + s1, b' = b + n a + s2 (mod 65521).  Each of the workgroup's LANES lanes folds a
// run of consecutive pieces from (a, b) = (0, 0); lane 0 then chains the runs, a run of n bytes adding n a to b.  Every product stays
// below 2^32.  Lane 0 alone calls done((b << 16) | a).
template <int PIECE, int LANES, typename Done>
__device__ __forceinline__ void adler_fold(const uint64_t* sums, int64_t npieces, int64_t N, Done&& done) {
    __shared__ uint32_t seg_a[LANES], seg_b[LANES], seg_n[LANES];
    const int tid = threadIdx.x;
    const int64_t per = (npieces + LANES - 1) / LANES;
    const int64_t c0 = min(npieces, tid * per), c1 = min(npieces, c0 + per);
    uint32_t A = 0, B = 0;
    for (int64_t c = c0; c < c1; ++c) {
        const uint64_t v = sums[c];
        const uint32_t n = (uint32_t)min((int64_t)PIECE, N - c * PIECE);
        B = (B + n * A + (uint32_t)(v >> 32)) % 65521u;
        A = (A + (uint32_t)v) % 65521u;
    }
    seg_a[tid] = A;
    seg_b[tid] = B;
    seg_n[tid] = (uint32_t)((min(N, c1 * PIECE) - min(N, c0 * PIECE)) % 65521);
    __syncthreads();
    if (tid == 0) {
        A = 1, B = 0;
        for (int t = 0; t < LANES; ++t) {
            B = (B + (uint32_t)(((uint64_t)seg_n[t] * A) % 65521u) + seg_b[t]) % 65521u;
            A = (A + seg_a[t]) % 65521u;
        }
        done((B << 16) | A);
    }
}

}  // namespace codec
}  // namespace nesr

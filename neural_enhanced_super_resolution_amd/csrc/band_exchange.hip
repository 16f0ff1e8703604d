// Row bands of one untiled frame on several contexts of one process (band_api.cpp: nesr_band_push_edges, nesr_forward_banded*):
// the apron exchange of banded.py without RCCL and without staging tensors.  After phase 0 of a dense block a band's first and last
// edge rows are final; one launch of band_push_edges reads them in the context's own activation layout and writes them, packed as
// nesr_band_rows packs them, into landing buffers that belong to the two neighbour contexts -- on the same device through the plain
// pointer, on another device through the peer mapping hipDeviceEnablePeerAccess gave the pointer (one address space: the same
// value).  Stands behind `self.model(img)` on a whole frame (nesr/nesr.py:887-891 with tile=0, nesr/nesr.py:224).
//
// The kernel is a gather copy: 16-byte loads, 16-byte stores, every store a vector store.  It waits for nothing and polls nothing:
// what a neighbour may read when is decided by HIP events on the host.
#include "nesr_kernels.h"

namespace nesr {

namespace {

__global__ __launch_bounds__(256) void band_push_edges(EdgePush a) {
    const int side = blockIdx.y;
    const char* __restrict__ src = a.src[side];
    char* __restrict__ dst = a.dst[side];
    if (!src) return;
    const unsigned per_seg = (unsigned)a.npieces * (unsigned)a.piece_vecs;
    const unsigned total = per_seg * (unsigned)a.nseg;          // < 2^31: the launcher checks
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        const unsigned seg = i / per_seg, r = i - seg * per_seg;
        const unsigned piece = r / (unsigned)a.piece_vecs, v = r - piece * (unsigned)a.piece_vecs;
        const uint4 val = *reinterpret_cast<const uint4*>(src + (long long)seg * a.seg_stride + (long long)piece * a.piece_stride + (long long)v * 16);
        *reinterpret_cast<uint4*>(dst + (size_t)i * 16) = val;
    }
}

}  // namespace

hipError_t launch_band_push_edges(const EdgePush& a, hipStream_t s) {
    if (!a.src[0] && !a.src[1]) return hipSuccess;
    const long long total = (long long)a.nseg * a.npieces * a.piece_vecs;
    if (a.nseg < 1 || a.npieces < 1 || a.piece_vecs < 1 || total >= (1ll << 31)) return hipErrorInvalidValue;
    if ((a.seg_stride | a.piece_stride) & 15) return hipErrorInvalidValue;
    for (int i = 0; i < 2; ++i)
        if (a.src[i] && (!a.dst[i] || ((reinterpret_cast<uintptr_t>(a.src[i]) | reinterpret_cast<uintptr_t>(a.dst[i])) & 15))) return hipErrorInvalidValue;
    long long blocks = (total + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(band_push_edges, dim3((unsigned)blocks, 2), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace nesr

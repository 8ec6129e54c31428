// gsr_scene_ops.hip — device-side scene editing (include/gsr.h "scene editing"): stable
// stream compaction of a keep mask into an index list, and the planar gather that builds a
// new scene block (or compacts a caller's per-Gaussian side arrays) from an index list.
#include "gsr_device.h"

namespace gsr {

namespace {

// ------------------------------------------------------------------ mask compaction
//
// d_indices[0 .. m) = the ascending i with keep[i] != 0.  The project's three-launch shape
// for a device-wide scan: per-chunk counts, one workgroup scanning the chunk counts, then
// ranks within each chunk and the writes.  A chunk is kMaskChunk mask bytes: 16 per thread,
// one 16-B load per lane when the mask is 16-B aligned (bytes otherwise, and in the tail).
constexpr int kMaskChunk = 256 * 16;      // mask bytes (items) per workgroup
constexpr int kMaskScanTile = 256 * 4;    // chunk counts the scan workgroup takes per iteration

// Bit 7 of every non-zero byte of w.
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t w) {
    return (((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u;
}

// Bit k set iff keep[i0 + k] != 0, k < 16; items at n and beyond read as 0.
__device__ __forceinline__ uint32_t mask_bits16(const uint8_t* __restrict__ keep, uint64_t i0, uint64_t n,
                                                bool vec) {
    if (i0 >= n) return 0u;
    uint32_t bits = 0;
    if (vec && i0 + 16 <= n) {
        const uint4 v = *reinterpret_cast<const uint4*>(keep + i0);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t z = nonzero_bytes(w[q]) >> 7;   // bits 0, 8, 16, 24
            bits |= ((z | (z >> 7) | (z >> 14) | (z >> 21)) & 0xfu) << (4 * q);
        }
    } else {
        const uint32_t cnt = (uint32_t)min((uint64_t)16, n - i0);
        for (uint32_t k = 0; k < cnt; k++) bits |= (keep[i0 + k] != 0 ? 1u : 0u) << k;
    }
    return bits;
}

__global__ __launch_bounds__(256) void k_mask_count(const uint8_t* __restrict__ keep, uint32_t n, bool vec,
                                                     uint32_t* __restrict__ counts) {
    __shared__ uint32_t s_scr[4];
    const uint64_t i0 = (uint64_t)blockIdx.x * kMaskChunk + threadIdx.x * 16u;
    const uint32_t c = (uint32_t)__popc(mask_bits16(keep, i0, n, vec));
    uint32_t tot;
    (void)block_exclusive_scan<uint32_t>(c, s_scr, tot);
    if (threadIdx.x == 0) counts[blockIdx.x] = tot;
}

// counts[0 .. chunks) -> their exclusive prefix sums, counts[chunks] = the total (m).
__global__ __launch_bounds__(256) void k_mask_scan(uint32_t* __restrict__ counts, uint32_t chunks) {
    __shared__ uint32_t s_scr[4];
    uint32_t carry = 0;
    for (uint32_t t0 = 0; t0 < chunks; t0 += kMaskScanTile) {
        const uint32_t b = t0 + threadIdx.x * 4u;
        uint32_t v[4], local = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            v[k] = b + k < chunks ? counts[b + k] : 0u;
            local += v[k];
        }
        uint32_t total;
        uint32_t run = carry + block_exclusive_scan<uint32_t>(local, s_scr, total);
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            if (b + k < chunks) counts[b + k] = run;
            run += v[k];
        }
        carry += total;
    }
    if (threadIdx.x == 0) counts[chunks] = carry;
}

// The chunk's kept indices are ranked into LDS and leave in coalesced runs.
__global__ __launch_bounds__(256) void k_mask_write(const uint8_t* __restrict__ keep, uint32_t n, bool vec,
                                                     const uint32_t* __restrict__ offs,
                                                     int32_t* __restrict__ indices) {
    __shared__ uint32_t s_scr[4];
    __shared__ int32_t s_idx[kMaskChunk];
    const uint64_t i0 = (uint64_t)blockIdx.x * kMaskChunk + threadIdx.x * 16u;
    uint32_t bits = mask_bits16(keep, i0, n, vec);
    uint32_t tot;
    uint32_t r = block_exclusive_scan<uint32_t>((uint32_t)__popc(bits), s_scr, tot);
    while (bits) {
        const uint32_t k = (uint32_t)__ffs(bits) - 1u;
        bits &= bits - 1u;
        s_idx[r++] = (int32_t)((uint32_t)i0 + k);
    }
    __syncthreads();
    // base + tot <= m <= n; the bound on n holds even if the caller changed the mask between
    // the count and this launch
    const uint32_t base = offs[blockIdx.x];
    for (uint32_t j = threadIdx.x; j < tot; j += 256)
        if ((uint64_t)base + j < n) indices[base + j] = s_idx[j];
}

// ------------------------------------------------------------------ planar gather
//
// dst[p * dst_stride + j] = src[p * src_stride + idx[j]], p < nplanes, j < m: the kernel that
// moves a scene (38 / 49 / 59 planes of 4-B elements) or a caller's side arrays.  The grid is
// j-chunks (x: one j per thread, so the index loads and every plane's stores are coalesced)
// by plane groups (y: kGatherGroup planes each).  A thread loads idx[j] once per plane group
// and walks the group in unrolled batches of kGatherBatch planes, every load of a batch
// issued before its first store: 8 loads x 4 B (8 B) x 2,048 resident threads keep 64 (128)
// KiB in flight per CU.  A monotone index list (a selection) reads each plane in near-
// coalesced runs; a random permutation pays one cache line per element and plane, which is
// inherent to the SoA layout.
//
// No address is formed from an unchecked index: an index outside [0, n) reads element
// min(max(idx, 0), n - 1), and the wave adds its count of such indices to *bad (nullable)
// with one atomic (plane group 0 only, so every index counts once).
//
// hdr (nullable): the new scene block's header, written by workgroup (0, 0) in stream order
// with the data (64 words: magic, count, stride, narrays, zeros).
constexpr int kGatherBatch = 8;
constexpr int kGatherGroup = 16;

struct SceneHeaderWords {
    uint32_t* dst;   // nullptr: no header
    uint64_t count, stride, narrays;
};

template <typename T, int K>
__device__ __forceinline__ void gather_batch(T* __restrict__ dst, const T* __restrict__ src, int64_t dst_stride,
                                             int64_t src_stride, int p, int64_t i, int64_t j) {
    T v[K];
#pragma unroll
    for (int k = 0; k < K; k++) v[k] = src[(int64_t)(p + k) * src_stride + i];
#pragma unroll
    for (int k = 0; k < K; k++) dst[(int64_t)(p + k) * dst_stride + j] = v[k];
}

template <typename T>
__global__ __launch_bounds__(256) void k_gather_planes(T* __restrict__ dst, int64_t dst_stride,
                                                        const T* __restrict__ src, int64_t src_stride, int nplanes,
                                                        uint32_t n, const int32_t* __restrict__ idx, uint32_t m,
                                                        uint32_t* __restrict__ bad, SceneHeaderWords hdr) {
    if (hdr.dst && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < GSR_SCENE_HEADER_BYTES / 4) {
        const uint32_t t = threadIdx.x;
        const uint64_t f = t < 6 ? hdr.count : t < 8 ? hdr.stride : hdr.narrays;
        uint32_t w = 0;
        if (t == 0) w = GSR_SCENE_MAGIC0;
        else if (t == 1) w = GSR_SCENE_MAGIC1;
        else if (t == 2) w = GSR_SCENE_MAGIC2;
        else if (t == 3) w = GSR_SCENE_MAGIC3;
        else if (t < 10) w = (t & 1u) ? (uint32_t)(f >> 32) : (uint32_t)f;
        hdr.dst[t] = w;
    }
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const bool valid = j < m;
    const int32_t r = valid ? idx[j] : 0;
    const bool oob = valid && (uint32_t)r >= n;   // negative indices wrap above n (n <= INT32_MAX)
    if (bad && blockIdx.y == 0) {
        const uint64_t b = __ballot(oob);
        if (b && lane_id() == 0) atomicAdd(bad, (uint32_t)__popcll(b));
    }
    if (!valid) return;
    const int64_t i = (int64_t)min(max(r, 0), (int32_t)(n - 1u));
    const int groups = (nplanes + kGatherGroup - 1) / kGatherGroup;
    for (int g = blockIdx.y; g < groups; g += gridDim.y) {
        int p = g * kGatherGroup;
        const int pend = min(p + kGatherGroup, nplanes);
        for (; p + kGatherBatch <= pend; p += kGatherBatch)
            gather_batch<T, kGatherBatch>(dst, src, dst_stride, src_stride, p, i, (int64_t)j);
        if (p + 4 <= pend) {
            gather_batch<T, 4>(dst, src, dst_stride, src_stride, p, i, (int64_t)j);
            p += 4;
        }
        if (p + 2 <= pend) {
            gather_batch<T, 2>(dst, src, dst_stride, src_stride, p, i, (int64_t)j);
            p += 2;
        }
        if (p < pend) gather_batch<T, 1>(dst, src, dst_stride, src_stride, p, i, (int64_t)j);
    }
}

}  // namespace

uint32_t mask_chunks(uint32_t n) { return (uint32_t)(((uint64_t)n + kMaskChunk - 1) / kMaskChunk); }

hipError_t launch_mask_indices(const uint8_t* keep, uint32_t n, uint32_t* counts, int32_t* indices, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint32_t chunks = mask_chunks(n);
    const bool vec = (reinterpret_cast<uintptr_t>(keep) & 15u) == 0;
    hipLaunchKernelGGL(k_mask_count, dim3(chunks), dim3(256), 0, s, keep, n, vec, counts);
    hipLaunchKernelGGL(k_mask_scan, dim3(1), dim3(256), 0, s, counts, chunks);
    hipLaunchKernelGGL(k_mask_write, dim3(chunks), dim3(256), 0, s, keep, n, vec, counts, indices);
    return hipGetLastError();
}

hipError_t launch_scan_counts(uint32_t* counts, uint32_t chunks, hipStream_t s) {
    hipLaunchKernelGGL(k_mask_scan, dim3(1), dim3(256), 0, s, counts, chunks);
    return hipGetLastError();
}

hipError_t launch_gather_planes(void* dst, int64_t dst_stride, const void* src, int64_t src_stride, int nplanes,
                                int elem_bytes, uint32_t n, const int32_t* idx, uint32_t m, uint32_t* bad,
                                void* scene_header, hipStream_t s) {
    if (m == 0 && !scene_header) return hipSuccess;
    const SceneHeaderWords hdr{static_cast<uint32_t*>(scene_header), m, (uint64_t)dst_stride, (uint64_t)nplanes};
    const int groups = (nplanes + kGatherGroup - 1) / kGatherGroup;
    const dim3 grid((uint32_t)std::max(1, grid_for(m, 256)), (uint32_t)(m ? std::min(groups, 65535) : 1));
    if (elem_bytes == 8)
        hipLaunchKernelGGL(k_gather_planes<uint64_t>, grid, dim3(256), 0, s, static_cast<uint64_t*>(dst), dst_stride,
                           static_cast<const uint64_t*>(src), src_stride, nplanes, n, idx, m, bad, hdr);
    else
        hipLaunchKernelGGL(k_gather_planes<uint32_t>, grid, dim3(256), 0, s, static_cast<uint32_t*>(dst), dst_stride,
                           static_cast<const uint32_t*>(src), src_stride, nplanes, n, idx, m, bad, hdr);
    return hipGetLastError();
}

}  // namespace gsr

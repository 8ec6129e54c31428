// gsr_scene_densify.hip — scene densification (include/gsr.h "scene densification"): the
// statistic the criterion reads, the stable expansion of a scene into kept, cloned and split
// Gaussians, the split children's arithmetic, the masked gather that cuts the Adam moments
// over, and the opacity reset.  The bulk move of the arrays is gsr_scene_ops.hip's planar
// gather on the expansion's source list; the chunk-count scan is its scan kernel too.
#include "gsr_preprocess_device.h"

namespace gsr {

namespace {

// ------------------------------------------------------------------ the statistic
//
// One thread owns one Gaussian: a plain load, add and store on its two words.  The only atomic
// is the wave's count of non-finite entries on *bad.
__global__ __launch_bounds__(256) void k_densify_accumulate(const float* __restrict__ center, uint32_t n, float hw,
                                                             float hh, float* __restrict__ accum,
                                                             uint32_t* __restrict__ seen, uint32_t* __restrict__ bad) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const bool valid = i < n;
    const float gx = valid ? center[i] : 0.0f;
    const float gy = valid ? center[(uint64_t)n + i] : 0.0f;
    const bool finite = fabsf(gx) < INFINITY && fabsf(gy) < INFINITY;   // false for NaN
    if (bad) {
        const uint64_t b = __ballot(valid && !finite);
        if (b && lane_id() == 0) atomicAdd(bad, (uint32_t)__popcll(b));
    }
    if (!valid || !finite || (gx == 0.0f && gy == 0.0f)) return;
    const float a = gx * hw;
    const float b = gy * hh;
    accum[i] += sqrtf((a * a) + (b * b));
    seen[i] += 1u;
}

// ------------------------------------------------------------------ the expansion
//
// The project's three-launch scan (gsr_scene_ops.hip "mask compaction") with 0, 1 or 2 outputs
// per item: k_densify_count classifies each source and writes its chunk's output count,
// launch_scan_counts turns the counts into the chunks' first output positions (and the total,
// n_out), k_densify_emit classifies again (six loads per source; a class byte per source kept
// in an n-byte scratch allocation measured slower: an all-kept densify of 5M Gaussians 0.63 ms
// against 0.44 ms, profiles/scene_densify.txt), ranks each chunk's outputs through LDS and
// writes the source and kind lists in coalesced runs.  A
// chunk is kDensifyChunk sources, kDensifyItems per thread in rounds (item r * 256 + t of the
// chunk for thread t), so every load is one contiguous run per wave; the four rounds' counts
// ride one block scan as 16-bit fields of a 64-bit word (a round's total is at most 512).
//
// A source's class: bits 0-1 the outputs (0, 1, 2), bit 2 set for a split.
constexpr int kDensifyItems = 4;
constexpr uint8_t kClassSplit = 4;

struct DensifyParams {
    float grad_threshold, scale_split, min_opacity, prune_scale_max, split_shrink;
};

// Fate of one source (include/gsr.h): float32 comparisons as written, NaNs compare false.
__device__ __forceinline__ uint8_t densify_class(float accum, uint32_t seen, float op, float s0, float s1, float s2,
                                                 const DensifyParams& P) {
    const float avg = seen ? accum / (float)seen : 0.0f;
    const bool hot = avg >= P.grad_threshold;
    const float smax = fmaxf(fmaxf(s0, s1), s2);
    const bool split = hot && smax > P.scale_split;
    const float sout = split ? smax / P.split_shrink : smax;
    const bool pruned = op < P.min_opacity || sout > P.prune_scale_max;
    if (pruned) return split ? kClassSplit : 0;
    return split ? (uint8_t)(kClassSplit | 2) : hot ? 2 : 1;
}

// The classes of the thread's kDensifyItems sources (0xff past n); every load is issued before
// the first class is formed.
struct DensifySource {
    const float* arrays;
    int64_t stride;
    uint32_t n;
    const float* accum;
    const uint32_t* seen;
};

__device__ __forceinline__ void densify_classes(const DensifySource& S, const DensifyParams& P,
                                                uint8_t (&c)[kDensifyItems]) {
    const float* __restrict__ op = S.arrays + (int64_t)GSR_A_OPACITY * S.stride;
    const float* __restrict__ sc = S.arrays + (int64_t)GSR_A_SCALE0 * S.stride;
    float a[kDensifyItems], o[kDensifyItems], s0[kDensifyItems], s1[kDensifyItems], s2[kDensifyItems];
    uint32_t sn[kDensifyItems];
    bool ok[kDensifyItems];
#pragma unroll
    for (int r = 0; r < kDensifyItems; r++) {
        const uint64_t i = (uint64_t)blockIdx.x * kDensifyChunk + (uint32_t)r * 256u + threadIdx.x;
        ok[r] = i < S.n;
        a[r] = ok[r] ? S.accum[i] : 0.0f;
        sn[r] = ok[r] ? S.seen[i] : 0u;
        o[r] = ok[r] ? op[i] : 0.0f;
        s0[r] = ok[r] ? sc[i] : 0.0f;
        s1[r] = ok[r] ? sc[S.stride + i] : 0.0f;
        s2[r] = ok[r] ? sc[2 * S.stride + i] : 0.0f;
    }
#pragma unroll
    for (int r = 0; r < kDensifyItems; r++)
        c[r] = ok[r] ? densify_class(a[r], sn[r], o[r], s0[r], s1[r], s2[r], P) : (uint8_t)0xff;
}

// totals: {kept, cloned, split, pruned} sources.
__global__ __launch_bounds__(256) void k_densify_count(DensifySource S, DensifyParams P,
                                                        uint32_t* __restrict__ counts,
                                                        uint32_t* __restrict__ totals) {
    __shared__ uint64_t s_scr[4];
    uint8_t c[kDensifyItems];
    densify_classes(S, P, c);
    uint64_t fates = 0;   // kept | cloned << 16 | split << 32 | pruned << 48
#pragma unroll
    for (int r = 0; r < kDensifyItems; r++) {
        if (c[r] == 0xff) continue;   // past n
        const uint32_t k = c[r] & 3u;
        fates += k == 0 ? 1ull << 48 : (c[r] & kClassSplit) ? 1ull << 32 : k == 2 ? 1ull << 16 : 1ull;
    }
    // a thread's fields are at most kDensifyItems: the block's sums (<= kDensifyChunk) fit 16 bits
    uint64_t tot;
    (void)block_exclusive_scan<uint64_t>(fates, s_scr, tot);
    if (threadIdx.x == 0) {
        uint32_t f[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            f[k] = (uint32_t)(tot >> (16 * k)) & 0xffffu;
            if (f[k]) atomicAdd(&totals[k], f[k]);
        }
        counts[blockIdx.x] = f[0] + 2u * (f[1] + f[2]);   // a kept source emits 1, a cloned or split one 2
    }
}

__global__ __launch_bounds__(256) void k_densify_emit(DensifySource S, DensifyParams P,
                                                       const uint32_t* __restrict__ offs, uint32_t n_out,
                                                       int32_t* __restrict__ src, uint8_t* __restrict__ kind) {
    __shared__ uint64_t s_scr[4];
    __shared__ int32_t s_src[2 * kDensifyChunk];
    __shared__ uint8_t s_kind[2 * kDensifyChunk];
    uint8_t c[kDensifyItems];
    densify_classes(S, P, c);
    uint64_t packed = 0;
#pragma unroll
    for (int r = 0; r < kDensifyItems; r++) {
        if (c[r] == 0xff) c[r] = 0;   // past n: no output
        packed |= (uint64_t)(c[r] & 3u) << (16 * r);
    }
    uint64_t tot;
    const uint64_t pre = block_exclusive_scan<uint64_t>(packed, s_scr, tot);
    uint32_t round_base = 0;
#pragma unroll
    for (int r = 0; r < kDensifyItems; r++) {
        const uint32_t k = c[r] & 3u;
        // round_base + rank + k <= the chunk's outputs <= 2 * kDensifyChunk
        const uint32_t at = round_base + ((uint32_t)(pre >> (16 * r)) & 0xffffu);
        const int32_t i = (int32_t)(blockIdx.x * (uint32_t)kDensifyChunk + (uint32_t)r * 256u + threadIdx.x);
        const uint8_t first = (c[r] & kClassSplit) ? 2 : 0;   // kinds 2, 3 | 0, 1
        if (k >= 1) {
            s_src[at] = i;
            s_kind[at] = first;
        }
        if (k == 2) {
            s_src[at + 1] = i;
            s_kind[at + 1] = (uint8_t)(first + 1);
        }
        round_base += (uint32_t)(tot >> (16 * r)) & 0xffffu;
    }
    __syncthreads();
    // base + round_base <= n_out when the statistic is the one the counts were taken from; the
    // bound holds even if the caller changed it between the count and this launch
    const uint32_t base = offs[blockIdx.x];
    for (uint32_t j = threadIdx.x; j < round_base; j += 256) {
        if ((uint64_t)base + j >= n_out) break;
        src[base + j] = s_src[j];
        kind[base + j] = s_kind[j];
    }
}

// ------------------------------------------------------------------ the split children
//
// One thread per output; kinds 2 and 3 overwrite the six planes the bulk move copied from the
// parent: s' = s / shrink, p'_r = p_r + ((R[r][0] t0 + R[r][1] t1) + R[r][2] t2), t_c = z_c s_c
// with the parent's scales and the child's normals (gsr_densify_normal3).
__global__ __launch_bounds__(256) void k_densify_split(float* __restrict__ dst, int64_t dst_stride, uint32_t n_out,
                                                        const float* __restrict__ arrays, int64_t stride, uint32_t n,
                                                        const int32_t* __restrict__ src,
                                                        const uint8_t* __restrict__ kind, float shrink, uint64_t seed) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= n_out) return;
    const uint32_t k = kind[j];
    if (k < 2u || k > 3u) return;
    const uint32_t i = (uint32_t)src[j];
    if (i >= n) return;   // never with the expansion's own lists
    auto A = [&](int a) { return arrays[(int64_t)a * stride + i]; };
    const float p[3] = {A(GSR_A_X), A(GSR_A_Y), A(GSR_A_Z)};
    const float s[3] = {A(GSR_A_SCALE0), A(GSR_A_SCALE0 + 1), A(GSR_A_SCALE0 + 2)};
    const float q[4] = {A(GSR_A_ROT0), A(GSR_A_ROT0 + 1), A(GSR_A_ROT0 + 2), A(GSR_A_ROT0 + 3)};
    float Rm[9], z[3];
    quat_rotation(q, Rm);
    gsr_densify_normal3(seed, i, k - 2u, z);
    const float t0 = z[0] * s[0], t1 = z[1] * s[1], t2 = z[2] * s[2];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        dst[(int64_t)(GSR_A_X + r) * dst_stride + j] = p[r] + ((Rm[3 * r] * t0 + Rm[3 * r + 1] * t1) + Rm[3 * r + 2] * t2);
        dst[(int64_t)(GSR_A_SCALE0 + r) * dst_stride + j] = s[r] / shrink;
    }
}

// ------------------------------------------------------------------ the masked moment gather
//
// dst[p][j] = kind[j] ? +0 : src[p][idx[j]]: k_gather_planes' mapping (one j per thread, plane
// groups in y) and its index rule — an index outside [0, n) that is read (kind 0) reads
// element min(max(idx, 0), n - 1) and counts into *bad, once (plane group 0).
constexpr int kMaskedGatherGroup = 8;

__global__ __launch_bounds__(256) void k_densify_gather(float* __restrict__ dst, int64_t dst_stride,
                                                         const float* __restrict__ srcp, int64_t src_stride,
                                                         int nplanes, uint32_t n, const int32_t* __restrict__ idx,
                                                         const uint8_t* __restrict__ kind, uint32_t m,
                                                         uint32_t* __restrict__ bad) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const bool valid = j < m;
    const bool fresh = valid && kind[j] != 0;
    const bool read = valid && !fresh && n > 0;
    const int32_t r = read ? idx[j] : 0;
    const bool oob = read && (uint32_t)r >= n;
    if (bad && blockIdx.y == 0) {
        const uint64_t b = __ballot(oob);
        if (b && lane_id() == 0) atomicAdd(bad, (uint32_t)__popcll(b));
    }
    if (!valid) return;
    const int64_t i = read ? (int64_t)min(max(r, 0), (int32_t)(n - 1u)) : 0;
    for (int p0 = blockIdx.y * kMaskedGatherGroup; p0 < nplanes; p0 += gridDim.y * kMaskedGatherGroup) {
        const int pend = min(p0 + kMaskedGatherGroup, nplanes);
        float v[kMaskedGatherGroup];
#pragma unroll
        for (int k = 0; k < kMaskedGatherGroup; k++)
            v[k] = (read && p0 + k < pend) ? srcp[(int64_t)(p0 + k) * src_stride + i] : 0.0f;
#pragma unroll
        for (int k = 0; k < kMaskedGatherGroup; k++)
            if (p0 + k < pend) dst[(int64_t)(p0 + k) * dst_stride + (int64_t)j] = v[k];
    }
}

// ------------------------------------------------------------------ the opacity reset
//
// o' = fminf(o, cap) for i < n, and the two moment planes (nullable) zeroed there.
__global__ __launch_bounds__(256) void k_reset_opacity(float* __restrict__ op, uint32_t n, float cap,
                                                        float* __restrict__ m_op, float* __restrict__ v_op) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    op[i] = fminf(op[i], cap);
    if (m_op) m_op[i] = 0.0f;
    if (v_op) v_op[i] = 0.0f;
}

}  // namespace

hipError_t launch_densify_accumulate(const float* center, uint32_t n, int W, int H, float* accum, uint32_t* seen,
                                     uint32_t* bad, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_densify_accumulate, dim3(grid_for(n, 256)), dim3(256), 0, s, center, n, 0.5f * (float)W,
                       0.5f * (float)H, accum, seen, bad);
    return hipGetLastError();
}

uint32_t densify_chunks(uint32_t n) { return (uint32_t)(((uint64_t)n + kDensifyChunk - 1) / kDensifyChunk); }

static DensifyParams densify_params(const gsr_densify_config& cfg) {
    return DensifyParams{cfg.grad_threshold, cfg.scale_split, cfg.min_opacity, cfg.prune_scale_max, cfg.split_shrink};
}

hipError_t launch_densify_count(const float* arrays, int64_t stride, uint32_t n, const float* accum,
                                const uint32_t* seen, const gsr_densify_config& cfg, uint32_t* counts,
                                uint32_t* totals, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint32_t chunks = densify_chunks(n);
    const DensifySource S{arrays, stride, n, accum, seen};
    hipLaunchKernelGGL(k_densify_count, dim3(chunks), dim3(256), 0, s, S, densify_params(cfg), counts, totals);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_scan_counts(counts, chunks, s);
}

hipError_t launch_densify_emit(const float* arrays, int64_t stride, uint32_t n, const float* accum,
                               const uint32_t* seen, const gsr_densify_config& cfg, const uint32_t* offs,
                               uint32_t n_out, int32_t* src, uint8_t* kind, hipStream_t s) {
    if (n == 0 || n_out == 0) return hipSuccess;
    const DensifySource S{arrays, stride, n, accum, seen};
    hipLaunchKernelGGL(k_densify_emit, dim3(densify_chunks(n)), dim3(256), 0, s, S, densify_params(cfg), offs, n_out,
                       src, kind);
    return hipGetLastError();
}

hipError_t launch_densify_split(float* dst, int64_t dst_stride, uint32_t n_out, const float* arrays, int64_t stride,
                                uint32_t n, const int32_t* src, const uint8_t* kind, float shrink, uint64_t seed,
                                hipStream_t s) {
    if (n_out == 0) return hipSuccess;
    hipLaunchKernelGGL(k_densify_split, dim3(grid_for(n_out, 256)), dim3(256), 0, s, dst, dst_stride, n_out, arrays,
                       stride, n, src, kind, shrink, seed);
    return hipGetLastError();
}

hipError_t launch_densify_gather(float* dst, int64_t dst_stride, const float* src, int64_t src_stride, int nplanes,
                                 uint32_t n, const int32_t* idx, const uint8_t* kind, uint32_t m, uint32_t* bad,
                                 hipStream_t s) {
    if (m == 0) return hipSuccess;
    const int groups = (nplanes + kMaskedGatherGroup - 1) / kMaskedGatherGroup;
    const dim3 grid((uint32_t)grid_for(m, 256), (uint32_t)std::min(groups, 65535));
    hipLaunchKernelGGL(k_densify_gather, grid, dim3(256), 0, s, dst, dst_stride, src, src_stride, nplanes, n, idx,
                       kind, m, bad);
    return hipGetLastError();
}

hipError_t launch_reset_opacity(float* arrays, int64_t stride, uint32_t n, float cap, float* m_op, float* v_op,
                                hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_reset_opacity, dim3(grid_for(n, 256)), dim3(256), 0, s,
                       arrays + (int64_t)GSR_A_OPACITY * stride, n, cap, m_op, v_op);
    return hipGetLastError();
}

}  // namespace gsr

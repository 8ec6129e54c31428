// gsr_probes.hip — device probes that belong to no stage: the rank-order self-check the
// runtime runs before it takes the returning-atomic rank path, and the math probe of the tests.
#include "gsr_device.h"

namespace gsr {

namespace {

// ------------------------------------------------------------------ rank-order self-check
//
// The RA rank path (match_peers' comment) relies on same-address ds_add_rtn_u32 lanes
// of one wave64 instruction returning the old values in lane order.  The runtime runs
// this check once per process and device before it uses that path: every wave of
// 256-thread workgroups (per-wave counters, as in the sort and binning kernels) ranks
// digits from 24 patterns — 1 to 256 distinct digits; uniform, a third of the lanes on
// one digit, runs of 16 lanes, interleaved; ~1/8 of the lanes idle — by returning
// atomics and by ballot matching, and counts the lanes where the two differ.
__device__ __forceinline__ uint32_t rank_check_hash(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

__global__ __launch_bounds__(256) void k_rank_order_check(uint32_t seed, int iters,
                                                           unsigned long long* __restrict__ out) {
    __shared__ uint32_t cnt[4][256];
    const uint32_t t = threadIdx.x, w = t >> 6, lane = t & 63u;
#pragma unroll
    for (int k = 0; k < 4; k++) cnt[k][t] = 0;
    __syncthreads();
    const uint64_t lt = lane ? (~0ull >> (64 - lane)) : 0ull;
    unsigned long long bad = 0, ops = 0;
    for (int pat = 0; pat < 24; pat++) {
        const int skew = pat / 6;
        constexpr uint32_t kDigits[6] = {1u, 2u, 4u, 16u, 128u, 256u};
        const uint32_t ndig = kDigits[pat % 6];
        for (int it = 0; it < iters; it++) {
            const uint32_t h = rank_check_hash(seed ^ (blockIdx.x * 7919u + (uint32_t)(pat * iters + it) * 104729u +
                                                       lane * 31u + w * 1000003u));
            uint32_t d = h % ndig;
            if (skew == 1) d = (h >> 8) % 3u == 0u ? 0u : d;
            if (skew == 2) d = (lane >> 4) % ndig;
            if (skew == 3) d = ((h >> 4) & 1u) ? (lane * 5u) % ndig : 1u % ndig;
            const bool valid = ((h >> 20) & 7u) != 0u;
            const uint64_t peers = match_peers<8>(d, valid, 8);
            uint32_t before = 0;
            if (valid) before = cnt[w][d];
            __builtin_amdgcn_wave_barrier();
            uint32_t got = 0;
            if (valid) got = atomicAdd(&cnt[w][d], 1u);
            __builtin_amdgcn_wave_barrier();
            if (valid) {
                bad += got != before + (uint32_t)__popcll(peers & lt);
                ops++;
            }
        }
    }
    // wave sums, one device atomic per wave
    for (int o = 32; o >= 1; o >>= 1) {
        bad += __shfl_xor(bad, o, 64);
        ops += __shfl_xor(ops, o, 64);
    }
    if (lane == 0) {
        atomicAdd(&out[0], ops);
        atomicAdd(&out[1], bad);
    }
}

// ------------------------------------------------------------------ math probe

__global__ void k_math_probe(const float* __restrict__ in, int n, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = in[2 * i], y = in[2 * i + 1];
    float* o = out + 9 * i;
    o[0] = gsr_expf(x);
    o[8] = gsr_blend_expf(x);
    o[1] = gsr_sinf(x);
    o[2] = gsr_cosf(x);
    o[3] = gsr_atan2f(x, y);
    o[4] = sqrtf(x);
    o[5] = x / y;
    o[6] = roundf(x);
    o[7] = __int_as_float(gsr_f2i_sat(x * 1000.0f));
}

}  // namespace

hipError_t rank_order_check(unsigned long long* lane_ops, unsigned long long* mismatches) {
    unsigned long long* d = nullptr;
    unsigned long long h[2] = {0, 0};
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&d), sizeof h);
    if (e != hipSuccess) return e;
    e = hipMemset(d, 0, sizeof h);
    // 1,024 workgroups (4 per CU) x 24 patterns x 8 iterations: ~44M lane-operations, well under 1 ms
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_rank_order_check, dim3(1024), dim3(256), 0, nullptr, 0x9E3779B9u, 8, d);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    *lane_ops = h[0];
    *mismatches = h[1];
    return e;
}

hipError_t launch_math_probe(const float* in, int n, float* out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_math_probe, dim3(grid_for(n, 256)), dim3(256), 0, s, in, n, out);
    return hipGetLastError();
}

}  // namespace gsr

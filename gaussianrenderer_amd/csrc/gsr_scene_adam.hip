// gsr_scene_adam.hip — the writer of a scene block besides the densification's opacity reset
// (include/gsr.h "scene optimisation"):
// a fused in-place Adam step over the block's arrays, from gsr_project_backward's gradient
// planes and the caller's moment planes.
#include "gsr_device.h"

namespace gsr {

namespace {

// One launch covers every active plane: the grid is element chunks (x) by active planes (y),
// so what differs between planes — the array it steps, its three caller planes, its learning
// rate and its update kind — is uniform per workgroup and sits in scalar registers, read from
// the plane table in the kernel arguments.
//
// A thread owns kAdamItems elements of its plane for the whole step (one owner per element, no
// atomics but *bad: reproducible bit for bit).  Two element mappings, chosen per plane:
//   wide   the plane's four pointers (block array, g, m, v) are all 16-B aligned: thread t owns
//          elements 4t .. 4t + 3 of the chunk and moves each as one 16-B access.  A block's
//          arrays always start 256-B aligned; a caller's [c*n + i] planes do when n is a
//          multiple of 4 (and the base is aligned).
//   narrow otherwise: thread t owns elements t, t + 256, t + 512, t + 768 of the chunk, so
//          every 4-B access of a wave is one contiguous 256-B run.
// The last, partial group of four of a wide plane is moved element by element.  Nothing at
// or past n is read or written in any plane, so the block's padding [n, stride) keeps its bits.
//
// Either way a dense thread issues its 16 dwords of loads (g, x, m, v) before the first use:
// 64 B x 2,048 resident threads = 128 KiB in flight per CU.  With SKIPZ the gradient is loaded
// first and a wave whose gradients are all +-0 leaves before it loads anything else: the
// visible-only step reads 4 B per element of what no pixel composited.
constexpr int kAdamItems = 4;
constexpr int kAdamThreads = 256;
constexpr uint32_t kAdamChunk = kAdamThreads * kAdamItems;

struct AdamSlots {
    uint32_t i[kAdamItems];   // element indices; i[0] .. i[0] + 3 when wide
    bool ok[kAdamItems];      // i[k] < n
    bool wide;                // one 16-B access covers the four
};

__device__ __forceinline__ void adam_load(const float* __restrict__ p, const AdamSlots& s, float (&o)[kAdamItems]) {
    if (s.wide) {
        const float4 t = *reinterpret_cast<const float4*>(p + s.i[0]);
        o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
    } else {
#pragma unroll
        for (int k = 0; k < kAdamItems; k++) o[k] = s.ok[k] ? p[s.i[k]] : 0.0f;
    }
}

// on[k]: the narrow path stores element k (the wide path stores all four: an element that
// is not stepped gets the bits it was loaded with).
__device__ __forceinline__ void adam_store(float* __restrict__ p, const AdamSlots& s, const float (&o)[kAdamItems],
                                           const bool (&on)[kAdamItems]) {
    if (s.wide) {
        *reinterpret_cast<float4*>(p + s.i[0]) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
        for (int k = 0; k < kAdamItems; k++)
            if (on[k]) p[s.i[k]] = o[k];
    }
}

// The arithmetic of include/gsr.h, one rounding per operation (the build has no contraction).
__device__ __forceinline__ void adam_element(int kind, float lr, const AdamLaunch& L, float g, float& x, float& m,
                                             float& v) {
    float gp = g;
    if (kind == kAdamOpacity) gp = g * (x * (1.0f - x));
    else if (kind == kAdamExp) gp = g * x;
    const float mn = (L.beta1 * m) + (L.omb1 * gp);
    const float vn = (L.beta2 * v) + ((L.omb2 * gp) * gp);
    const float d = (lr * (mn / L.bc1)) / (sqrtf(vn / L.bc2) + L.eps);
    float xn;
    if (kind == kAdamOpacity) {
        xn = x / (x + (1.0f - x) * gsr_expf(d));
        xn = fminf(fmaxf(xn, GSR_ADAM_OPACITY_MIN), GSR_ADAM_OPACITY_MAX);
    } else if (kind == kAdamExp) {
        xn = x * gsr_expf(-d);
    } else {
        xn = x - d;
    }
    x = xn;
    m = mn;
    v = vn;
}

template <bool SKIPZ, bool ZEROG>
__global__ __launch_bounds__(kAdamThreads) void k_scene_adam(float* __restrict__ arrays, int64_t stride, uint32_t n,
                                                              const AdamLaunch L, uint32_t* __restrict__ bad) {
    const AdamPlane pl = L.plane[blockIdx.y];
    float* __restrict__ x_p = arrays + (int64_t)pl.array * stride;
    const bool aligned = ((reinterpret_cast<uintptr_t>(x_p) | reinterpret_cast<uintptr_t>(pl.g) |
                           reinterpret_cast<uintptr_t>(pl.m) | reinterpret_cast<uintptr_t>(pl.v)) & 15u) == 0;
    // n <= INT32_MAX: every index below stays under 2^31 + kAdamChunk
    const uint32_t base = blockIdx.x * kAdamChunk;
    AdamSlots s;
    s.wide = aligned && base + threadIdx.x * kAdamItems + kAdamItems <= n;
#pragma unroll
    for (int k = 0; k < kAdamItems; k++) {
        s.i[k] = aligned ? base + threadIdx.x * kAdamItems + k : base + k * kAdamThreads + threadIdx.x;
        s.ok[k] = s.i[k] < n;
    }

    float g[kAdamItems], x[kAdamItems], m[kAdamItems], v[kAdamItems];
    adam_load(pl.g, s, g);
    if (SKIPZ) {
        bool any = false;
#pragma unroll
        for (int k = 0; k < kAdamItems; k++) any |= s.ok[k] && !(g[k] == 0.0f);
        if (__ballot(any) == 0) return;   // nothing to step, nothing to count, nothing to clear
    }
    adam_load(x_p, s, x);
    adam_load(pl.m, s, m);
    adam_load(pl.v, s, v);

    bool on[kAdamItems], clear[kAdamItems];
    bool any_on = false, any_clear = false;
    uint32_t nbad = 0;
#pragma unroll
    for (int k = 0; k < kAdamItems; k++) {
        const bool finite = fabsf(g[k]) < INFINITY;   // false for NaN
        const bool isbad = s.ok[k] && !finite;
        nbad += (uint32_t)__popcll(__ballot(isbad));
        on[k] = s.ok[k] && finite && !(SKIPZ && g[k] == 0.0f);
        clear[k] = s.ok[k] && !(g[k] == 0.0f);         // already +-0: reads as cleared
        any_on |= on[k];
        any_clear |= clear[k];
        if (on[k]) adam_element(pl.kind, pl.lr, L, g[k], x[k], m[k], v[k]);
    }
    if (bad && nbad && lane_id() == 0) atomicAdd(bad, nbad);
    if (any_on) {
        adam_store(x_p, s, x, on);
        adam_store(pl.m, s, m, on);
        adam_store(pl.v, s, v, on);
    }
    if (ZEROG && any_clear) {
        const float z[kAdamItems] = {0.0f, 0.0f, 0.0f, 0.0f};
        adam_store(pl.g, s, z, clear);
    }
}

}  // namespace

hipError_t launch_scene_adam(float* arrays, int64_t stride, uint32_t n, const AdamLaunch& L, uint32_t* bad,
                             hipStream_t s) {
    if (n == 0 || L.nplanes <= 0) return hipSuccess;
    const dim3 grid((uint32_t)grid_for(n, (int)kAdamChunk), (uint32_t)L.nplanes);
    const bool skipz = (L.flags & GSR_ADAM_SKIP_ZERO) != 0, zerog = (L.flags & GSR_ADAM_ZERO_GRADS) != 0;
    with_bool(skipz, [&](auto sz) {
        with_bool(zerog, [&](auto zg) {
            hipLaunchKernelGGL((k_scene_adam<decltype(sz)::value, decltype(zg)::value>), grid, dim3(kAdamThreads), 0,
                               s, arrays, stride, n, L, bad);
            return 0;
        });
        return 0;
    });
    return hipGetLastError();
}

}  // namespace gsr

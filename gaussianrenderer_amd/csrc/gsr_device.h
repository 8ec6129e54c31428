// gsr_device.h — device helpers the gfx950 kernel translation units share (gsr_kernels.hip,
// gsr_bucket_sort.hip, gsr_blend.hip, gsr_blend_derived.hip, gsr_scene_ops.hip, gsr_scene_densify.hip, gsr_scene_init.hip, gsr_scene_pack.hip, gsr_image_loss.hip,
// gsr_project.hip, gsr_probes.hip): wave and workgroup
// scans, ballot ranking, chunk and XCD mappings, the depth-sort pass plan, and the host-side
// launch helpers.  Inline functions only: no kernels, no __constant__ data.  What only the
// blend kernels share is in gsr_blend_device.h, what only the geometry stages share in
// gsr_geom_device.h.
#pragma once

#include <hip/hip_runtime.h>
#include <algorithm>
#include <type_traits>

#include "gsr_detmath.h"
#include "gsr.h"
#include "gsr_internal.h"

namespace gsr {

namespace {

// Geometry kernels raise their waves' instruction-issue priority (s_setprio) above
// the blend's: with frames in flight, a geometry wave that shares a SIMD with blend
// waves would otherwise queue behind them for the VALU.  Issue priority only: no
// preemption, no effect on a kernel running alone (+0.8 % frames/s in flight,
// interleaved A/B of two builds: profiles/r02_ab_setprio.txt).
#ifndef GSR_GEOM_PRIORITY
#define GSR_GEOM_PRIORITY 3
#endif
#define GSR_GEOM_PRIO()                                                            \
    do {                                                                           \
        if (GSR_GEOM_PRIORITY > 0) __builtin_amdgcn_s_setprio(GSR_GEOM_PRIORITY); \
    } while (0)

__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }

// Cross-lane moves on the DPP path (VALU) instead of ds_bpermute (the LDS crossbar,
// one LDS round trip per step): a wave64 scan is six dependent VALU ops.  CDNA4 is a
// GFX9 core, so row_bcast:15 / :31 and wave_shr:1 exist.  Lanes a control does not
// reach (row start for row_shr, rows outside row_mask) read 0, the identity of every
// scan below (add, unsigned max, or).
template <int CTRL, int ROWM, bool BC>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t x) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, ROWM, 0xf, BC);
}
template <int CTRL, int ROWM, bool BC, typename T>
__device__ __forceinline__ T dpp_mov(T x) {
    if constexpr (sizeof(T) == 4) {
        return (T)dpp_u32<CTRL, ROWM, BC>((uint32_t)x);
    } else {
        const uint64_t u = (uint64_t)x;
        const uint32_t lo = dpp_u32<CTRL, ROWM, BC>((uint32_t)u), hi = dpp_u32<CTRL, ROWM, BC>((uint32_t)(u >> 32));
        return (T)(((uint64_t)hi << 32) | lo);
    }
}
struct OpAdd {
    template <typename T>
    __device__ T operator()(T a, T b) const { return a + b; }
};
struct OpMax {
    __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return max(a, b); }
};
struct OpOr {
    __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a | b; }
};
// Inclusive wave64 scan: Hillis-Steele inside each row of 16 lanes (row_shr 1, 2, 4, 8),
// then row 0's total into row 1 and row 2's into row 3 (row_bcast:15), then rows 0-1's
// into rows 2-3 (row_bcast:31).
template <typename T, typename Op>
__device__ __forceinline__ T wave_incl_scan(T x, Op op) {
    x = op(x, dpp_mov<0x111, 0xf, true>(x));
    x = op(x, dpp_mov<0x112, 0xf, true>(x));
    x = op(x, dpp_mov<0x114, 0xf, true>(x));
    x = op(x, dpp_mov<0x118, 0xf, true>(x));
    x = op(x, dpp_mov<0x142, 0xa, false>(x));
    x = op(x, dpp_mov<0x143, 0xc, false>(x));
    return x;
}
// The value of the lane below (0 at lane 0): wave_shr:1.
__device__ __forceinline__ uint32_t wave_shr1(uint32_t x) { return dpp_u32<0x138, 0xf, true>(x); }

// Exclusive scan across a workgroup of NW waves (4 = 256 threads unless a kernel says
// otherwise); `scratch` holds NW entries.  Contains two barriers; every thread of the
// block must call it.
template <typename T, int NW = 4>
__device__ __forceinline__ T block_exclusive_scan(T v, T* scratch, T& total) {
    const uint32_t lane = lane_id();
    const uint32_t w = threadIdx.x >> 6;
    const T x = wave_incl_scan(v, OpAdd{});
    if (lane == 63) scratch[w] = x;
    __syncthreads();
    T pre = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < NW; k++) {
        const T s = scratch[k];
        if ((uint32_t)k < w) pre += s;
        tot += s;
    }
    __syncthreads();
    total = tot;
    return pre + x - v;
}

// block_exclusive_scan without its trailing barrier: the caller barriers before `scratch`
// is written again (and before anything it publishes from the result is read).
template <typename T, int NW = 4>
__device__ __forceinline__ T block_exclusive_scan_lead(T v, T* scratch, T& total) {
    const uint32_t lane = lane_id();
    const uint32_t w = threadIdx.x >> 6;
    const T x = wave_incl_scan(v, OpAdd{});
    if (lane == 63) scratch[w] = x;
    __syncthreads();
    T pre = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < NW; k++) {
        const T s = scratch[k];
        if ((uint32_t)k < w) pre += s;
        tot += s;
    }
    total = tot;
    return pre + x - v;
}

// Wave64-wide max / or (every lane gets the result: lane 63 of the inclusive scan).
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan(v, OpMax{}), 63);
}
__device__ __forceinline__ uint32_t wave_or_u32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan(v, OpOr{}), 63);
}

// [begin, end) of workgroup g when n items are split over `groups` workgroups in
// chunks that are multiples of `gran`.
__device__ __forceinline__ void chunk_range(uint64_t n, int groups, int g, uint64_t gran,
                                            uint64_t& b, uint64_t& e) {
    uint64_t per = (n + (uint64_t)groups - 1) / (uint64_t)groups;
    per = (per + gran - 1) / gran * gran;
    b = per * (uint64_t)g;
    if (b > n) b = n;
    e = b + per;
    if (e > n) e = n;
}

// Chunk handled by workgroup b of G when the chunks are dealt so that each XCD
// takes one contiguous run of them (a bijection on [0, G); hardware dispatch sends
// workgroup b to XCD b mod 8).  The partial cache lines at the seams between
// consecutive chunks' output runs are then written through one L2.  Used by the
// depth sort's downsweep at 16 items per thread (scenes of 4M+ Gaussians: config
// 3 depth sort 173 -> 163 us); not by the binning scatters, whose chunks carry
// uneven work (near splats cover more rows and columns) that contiguous runs would
// pile onto one XCD (config 3 rows 100 -> 143 us, columns 143 -> 199 us;
// profiles/r02_ab_xcd_chunks.txt).  The blend maps its blocks the same way (blend_block_index):
// blocks that share an XCD get one contiguous run of tiles, so neighbouring tiles' shared
// splats hit one L2.
#ifndef GSR_XCD_DEPTH
#define GSR_XCD_DEPTH 1   // 0: round-robin chunks in the depth downsweep too (A/B builds)
#endif
__device__ __forceinline__ int xcd_chunk(int b, int G) {
    const int xcd = b & 7, q = G >> 3, r = G & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (b >> 3);
}

// Lanes of the wave whose `bits`-bit digit equals this lane's, among the lanes in
// `valid` (the wave64 stand-in for __match_any): one ballot per digit bit.  Per bit
// 4 VALU: v_bfe_i32 (the bit as a 0 / -1 mask m), the ballot's v_cmp, and one
// v_bitop3_b32 per mask half computing peers & ~(ballot ^ m) — truth table 0x90 for
// (peers, ballot, m), index S0*4 + S1*2 + S2 (tools/microbench/bitop3_probe.hip) —
// where the select-and-mask form compiles to 8.
// (MAXB: compile-time bound on `bits`, so the loop unrolls; bits <= MAXB.)
//
// The alternative, stable in-wave ranks from returning LDS atomics (template flag RA, runtime
// knob GSR_TUNE_RANK_ATOMIC): atomicAdd(&count[digit], 1) from one wave64 instruction
// returns the old values in LANE order when several lanes hit one address — measured
// on gfx950 with no exception in 1.5e10 lane-operations over uniform, skewed, run and
// interleaved digit patterns (tools/microbench/lds_atomic_order.hip) — so the returned
// value is the element's stable rank among the wave's earlier elements of its digit:
// one LDS op instead of ballot matching (4 VALU per digit bit).  The ISA
// does not document that order, so the runtime only takes RA = true after
// k_rank_order_check (gsr_probes.hip) has found it on the device in this process; otherwise,
// or with the knob at 0, every kernel ranks with ballots (RA = false).
template <int MAXB>
__device__ __forceinline__ uint64_t match_peers(uint32_t d, bool valid, int bits) {
    const uint64_t v = __ballot(valid);
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
#pragma unroll
    for (int bit = 0; bit < MAXB; bit++) {
        if (bit >= bits) break;
        const int m = __builtin_amdgcn_sbfe((int)d, bit, 1);
        const uint64_t bm = __ballot(m != 0);
        lo = __builtin_amdgcn_bitop3_b32(lo, (uint32_t)bm, (uint32_t)m, 0x90);
        hi = __builtin_amdgcn_bitop3_b32(hi, (uint32_t)(bm >> 32), (uint32_t)m, 0x90);
    }
    return ((uint64_t)hi << 32) | lo;
}

// math.cu:131-138 (matVecMul4D_cuda).
__device__ __forceinline__ void mv4(const float* M, const float* v, float* out) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j) acc += M[i * 4 + j] * v[j];
        out[i] = acc;
    }
}

// Depth-sort pass plan.  dstats (zeroed per frame, filled by pass 0's upsweep
// over every key except 0xFFFFFFFF, which culled records carry): [0] max of ~key
// (= ~min key), [1] max key, [2] bit p set if some key has its low 8p bits all
// ones, [3] nonzero if any such key exists.  Pass p >= 1 is an identity (and is
// skipped) when every key shares the digits at and above p and no key has
// all-ones low 8p bits: the 0xFFFFFFFF keys then already trail in index order,
// exactly where the full sort puts them.  Skippable(p) implies skippable(p+1).
__device__ __forceinline__ bool depth_pass_skipped(const uint32_t* __restrict__ dstats, int pass) {
    if (!dstats || pass == 0) return false;
    if (dstats[3] == 0u) return true;
    const uint32_t kmin = ~dstats[0], kmax = dstats[1];
    return (kmin >> (8 * pass)) == (kmax >> (8 * pass)) && !((dstats[2] >> pass) & 1u);
}

__device__ __forceinline__ int depth_passes_run(const uint32_t* __restrict__ dstats) {
    int p = 1;
    while (p < 4 && !depth_pass_skipped(dstats, p)) ++p;
    return p;
}

// The depth sort ends in items[passes run & 1] (trailing identity passes are
// skipped on the device).
__device__ __forceinline__ const uint64_t* depth_sorted(const uint64_t* items0, const uint64_t* items1,
                                                        const uint32_t* dstats) {
    return (depth_passes_run(dstats) & 1) ? items1 : items0;
}

// f(std::true_type{}) or f(std::false_type{}): a runtime bool as a template argument of the
// launches in the generic lambda f.
template <typename F>
inline auto with_bool(bool b, F&& f) {
    return b ? f(std::true_type{}) : f(std::false_type{});
}

// f(std::integral_constant<int, v>{}) for a runtime v in [1, 15], nothing for any other v: a
// runtime set of output bits as a template argument of the launch in the generic lambda f.
template <int V = 1, typename F>
inline void with_int_1_15(int v, F&& f) {
    if constexpr (V <= 15) {
        if (v == V) f(std::integral_constant<int, V>{});
        else with_int_1_15<V + 1>(v, f);
    }
}

inline int grid_for(int64_t n, int block) { return (int)((n + block - 1) / block); }

}  // namespace

}  // namespace gsr

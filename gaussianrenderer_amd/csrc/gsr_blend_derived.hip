// gsr_blend_derived.hip — the passes derived from the exact blend (gfx950, CDNA4): k_blend_aux
// (gsr_render_aux), k_blend_contrib (gsr_render_contrib), k_blend_backward
// (gsr_render_backward) and k_blend_backward_aux (gsr_render_backward_aux), with the
// per-Gaussian kernels that feed them.  Each walks a block's
// list with the functions of gsr_blend_device.h — k_blend_w's schedule, cull and exact
// one-splat step (gsr_blend.hip) — and owns only its LDS slot layout, what it accumulates per
// take and its epilogue (k_blend_aux also its copy of the record load and prefetch).  Compiled like gsr_blend.hip: -ffp-contract=off, gsr_detmath.h.
#include "gsr_blend_device.h"

namespace gsr {

namespace {

// -Z of every Gaussian (gsr_render_aux's depth channel): Z is the view-space z of
// preprocess_one — the same position (4D: at tnow, the same expression) through the same
// mv4 — so -Z is the float whose scaled value becomes the depth key, the positive distance
// along the view axis.  Culled Gaussians get whatever the product gives; no list holds them.
template <bool T4D>
__global__ __launch_bounds__(256) void k_aux_depth(const float* __restrict__ arr, int64_t stride, int64_t n,
                                                   Frame fr, float tnow, float* __restrict__ z) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    auto A = [&](int64_t k) { return arr[k * stride + i]; };
    float gx = A(GSR_A_X);
    float gy = A(GSR_A_Y);
    float gz = A(GSR_A_Z);
    if (T4D) {
        const float dt = tnow - A(GSR_A_TCENTER);
        const float dt2 = dt * dt, dt3 = dt2 * dt;
        auto m = [&](int j) { return A(GSR_A_MOTION0 + j); };
        gx = ((gx + m(0) * dt) + m(3) * dt2) + m(6) * dt3;
        gy = ((gy + m(1) * dt) + m(4) * dt2) + m(7) * dt3;
        gz = ((gz + m(2) * dt) + m(5) * dt2) + m(8) * dt3;
    }
    const float old_xyz[4] = {gx, gy, gz, 1.0f};
    float tmp_xyz[4];
    mv4(fr.V, old_xyz, tmp_xyz);
    z[i] = -tmp_xyz[2];
}

// The 8-channel kernel's feature values interleaved per Gaussian: pack[2 i] and pack[2 i + 1]
// hold features 0-3 and 4-7 of Gaussian i (0 from nfeat on).  The arrays are planar and the
// blend gathers by scattered Gaussian index, so each planar value costs a survivor a cache
// line of its own; interleaved, its eight values are one 32-B piece of one line.  Coalesced
// both ways (4 nfeat + 32 bytes per Gaussian).
__global__ __launch_bounds__(256) void k_aux_pack(const float* __restrict__ features, int64_t n, int nfeat,
                                                  float4* __restrict__ pack) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float v[8];
#pragma unroll
    for (int f = 0; f < 8; f++) v[f] = f < nfeat ? features[(int64_t)f * n + i] : 0.0f;
    pack[2 * i] = make_float4(v[0], v[1], v[2], v[3]);
    pack[2 * i + 1] = make_float4(v[4], v[5], v[6], v[7]);
}

// Where k_blend_aux reads its per-Gaussian values and writes its planes (nullable each;
// feat / features with nfeat > 0).
struct AuxIO {
    float* color;            // 3 planes
    float* alpha;
    float* depth;
    float* feat;             // nfeat planes
    const float* features;   // nfeat arrays of n floats (NF = 4)
    const float4* pack;      // k_aux_pack's output (NF = 8)
    const float* z;          // k_aux_depth's output (depth != nullptr)
    int64_t n;
    int nfeat;
};

// The blend with auxiliary targets (gsr_render_aux): k_blend_w's schedule — one wave64 per
// 8x8 block, one-wave workgroups, the same block -> workgroup mapping and tile lists, the
// same 64-record batches, prefetch and conservative cull (gsr_blend_device.h) — and, for every
// survivor, the exact one-splat step of blend_block (splat_step), so each pixel takes the
// decisions of render.cu:323-341 and the colours are the exact blend's bit for bit.  Every other channel accumulates like a colour, acc = fma(v alpha, T, acc)
// in list order: v = 1 (alpha: the accumulated coverage), v = -Z (depth, un-normalised)
// and v = the Gaussian's feature values.  Only a surviving lane gathers its splat's -Z
// and features (by Gaussian index; the records do not hold them): up to four from the
// planar arrays, more from k_aux_pack's interleaved copy.
//
// Survivor k's slot in the wave's LDS slice (12 + NF dwords, 16-B aligned, read with
// wave-uniform addresses):
//   [0] cx [1] cy [2] a [3] b | [4] c [5] e [6] opacity [7] red | [8] green [9] blue
//   [10] -Z [11] unused | [12 ..] features
// NF = 0 / 4 / 8: 3 / 4 / 5 KiB per wave.  Eight waves per SIMD of NF = 8 would need the
// CU's whole 160 KiB and squeeze its 13 accumulators into 64 VGPRs, so that instantiation
// asks for six or more (with colour it compiles to 69 VGPRs: seven waves, 140 KiB, no spill); the
// others keep k_blend_w's eight.
// COLOR false: no colour planes (the colour accumulations drop out).
template <int NF, bool COLOR>
__global__ __launch_bounds__(64, NF > 4 ? 6 : 8) void k_blend_aux(const uint32_t* __restrict__ idx,
                                                                 const uint2* __restrict__ ranges,
                                                                 const uint4* __restrict__ rec, int tiles_x,
                                                                 int tiles_y, int W, int H, int cover_w,
                                                                 int cover_h, int bands, AuxIO io) {
    constexpr int kSlot = 12 + NF;                          // dwords per survivor slot
    constexpr int kNF = NF ? NF : 1;
    __shared__ float4 sP[64 * kSlot / 4];
    BlockSetup bs;
    if (!block_setup(bs, ranges, tiles_x, tiles_y, cover_w, cover_h, bands)) return;
    const uint32_t beg = bs.beg, end = bs.end;
    const int lane = bs.lane, px = bs.px, py = bs.py;
    const bool inside = bs.inside;
    const float fpx = bs.fpx, fpy = bs.fpy;
    const float4* wP4 = sP;

    // pixels outside the covered area start saturated and write 0 (blend_block)
    float T = inside ? 1.0f : 0.0f;
    float cr = 0.0f, cg = 0.0f, cb = 0.0f, ca = 0.0f, cz = 0.0f, cf[kNF];
#pragma unroll
    for (int f = 0; f < kNF; f++) cf[f] = 0.0f;

    // the record batch (RecordBatch) in plain locals, loaded and prefetched here as batch_first
    // and batch_prefetch do it: behind those two functions this kernel's register figures move
    // and its 4-channel instantiation runs about 1 % slower (gsr_blend_device.h)
    uint4 ra = make_uint4(0, 0, 0, 0), rb = ra, rc = ra, rd = ra;
    uint32_t nidx = 0, cidx = 0;
    if (beg + lane < end) {
        cidx = idx[beg + lane];
        const uint4* R = rec + 4 * (uint64_t)cidx;
        ra = R[0];
        rb = R[1];
        rc = R[2];
        rd = R[3];
    }
    if (beg + 64 + lane < end) nidx = idx[beg + 64 + lane];
    bool alive = __ballot(!(T < 1e-3f)) != 0ull;
    for (uint32_t base = beg; base < end && alive; base += 64) {
        const uint32_t cnt = min(64u, end - base);
        // ---- cull (lane = record) ----
        BlockCull cl;
        const bool hit = block_cull(cl, ra, rc, rd, bs.bx, bs.by, lane, cnt, __ballot(!(T < 1e-3f)));
        const uint32_t dsc = cl.dsc;
        // ---- survivors, compacted in list order; each gathers its -Z and features ----
        const uint64_t m = __ballot(hit);
        const uint32_t k_l = ballot_rank(m);
        float zv = 0.0f, fv[kNF];
#pragma unroll
        for (int f = 0; f < kNF; f++) fv[f] = 0.0f;
        if (hit) {
            if (io.z) zv = io.z[cidx];
            if (NF == 8) {
                const float4 p0 = io.pack[2 * (int64_t)cidx], p1 = io.pack[2 * (int64_t)cidx + 1];
                fv[0] = p0.x; fv[1 % kNF] = p0.y; fv[2 % kNF] = p0.z; fv[3 % kNF] = p0.w;
                fv[4 % kNF] = p1.x; fv[5 % kNF] = p1.y; fv[6 % kNF] = p1.z; fv[7 % kNF] = p1.w;
            } else {
#pragma unroll
                for (int f = 0; f < NF; f++)   // padding channels repeat the last array (never stored)
                    fv[f] = io.features[(int64_t)min(f, io.nfeat - 1) * io.n + (int64_t)cidx];
            }
            float4* S4 = sP + k_l * (kSlot / 4);
            S4[0] = make_float4(__uint_as_float(rc.x), __uint_as_float(rc.y), __uint_as_float(ra.x),
                                __uint_as_float(ra.y));
            S4[1] = make_float4(__uint_as_float(ra.z), __uint_as_float(ra.w), __uint_as_float(rb.x),
                                __uint_as_float(rb.y));
        }
        const float col_g = __uint_as_float(rb.z), col_b = __uint_as_float(rb.w);
        // ---- prefetch: records of batch k+1, indices of batch k+2 (batch_prefetch) ----
        if (base + 64 + lane < end) {
            cidx = nidx;
            const uint4* R = rec + 4 * (uint64_t)nidx;
            ra = R[0];
            rb = R[1];
            rc = R[2];
            rd = R[3];
        }
        if (base + 128 + lane < end) nidx = idx[base + 128 + lane];
        if (hit) {
            // (the gathered values last: their loads were issued ahead of the prefetch)
            float4* S4 = sP + k_l * (kSlot / 4);
            S4[2] = make_float4(col_g, col_b, zv, 0.0f);
            if (NF >= 4) S4[3] = make_float4(fv[0], fv[1 % kNF], fv[2 % kNF], fv[3 % kNF]);
            if (NF >= 8) S4[4] = make_float4(fv[4 % kNF], fv[5 % kNF], fv[6 % kNF], fv[7 % kNF]);
        }
        // ---- the exact one-splat step over the survivors (render.cu:329-340) ----
        uint64_t mm = m;
        for (uint32_t k = 0; mm && alive; ++k) {
            const int s = __builtin_ctzll(mm);
            mm &= mm - 1;
            const uint64_t box = box_mask((uint32_t)__builtin_amdgcn_readlane((int)dsc, s));
            const float4 q0 = wP4[k * (kSlot / 4) + 0], q1 = wP4[k * (kSlot / 4) + 1];
            const float4 q2 = wP4[k * (kSlot / 4) + 2];
            SplatStep st;
            const bool take = splat_step(st, fpx, fpy, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, box, T);
            const float alpha = st.alpha;
            if (COLOR) {
                const float wr = __builtin_fmaf(q1.w * alpha, T, cr);
                const float wg = __builtin_fmaf(q2.x * alpha, T, cg);
                const float wb = __builtin_fmaf(q2.y * alpha, T, cb);
                cr = take ? wr : cr;
                cg = take ? wg : cg;
                cb = take ? wb : cb;
            }
            // alpha's value is 1.0f: 1.0f * alpha is alpha exactly
            const float wa = __builtin_fmaf(alpha, T, ca);
            const float wz = __builtin_fmaf(q2.z * alpha, T, cz);
            ca = take ? wa : ca;
            cz = take ? wz : cz;
            if (NF >= 4) {
                const float4 q3 = wP4[k * (kSlot / 4) + 3];
                const float v[4] = {q3.x, q3.y, q3.z, q3.w};
#pragma unroll
                for (int f = 0; f < 4; f++) {
                    const float wf = __builtin_fmaf(v[f] * alpha, T, cf[f % kNF]);
                    cf[f % kNF] = take ? wf : cf[f % kNF];
                }
            }
            if (NF >= 8) {
                const float4 q4 = wP4[k * (kSlot / 4) + 4];
                const float v[4] = {q4.x, q4.y, q4.z, q4.w};
#pragma unroll
                for (int f = 0; f < 4; f++) {
                    const float wf = __builtin_fmaf(v[f] * alpha, T, cf[(4 + f) % kNF]);
                    cf[(4 + f) % kNF] = take ? wf : cf[(4 + f) % kNF];
                }
            }
            const float Tn = T * (1.0f - alpha);
            T = take ? Tn : T;
            alive = __ballot(!(T < 1e-3f)) != 0ull;
        }
    }
    if (px < W && py < H) {
        const size_t o = (size_t)py * (size_t)W + (size_t)px;
        const size_t hw = (size_t)W * (size_t)H;
        if (COLOR) {
            io.color[o] = inside ? cr : 0.0f;
            io.color[hw + o] = inside ? cg : 0.0f;
            io.color[2 * hw + o] = inside ? cb : 0.0f;
        }
        if (io.alpha) io.alpha[o] = inside ? ca : 0.0f;
        if (io.depth) io.depth[o] = inside ? cz : 0.0f;
#pragma unroll
        for (int f = 0; f < NF; f++)
            if (f < io.nfeat) io.feat[(size_t)f * hw + o] = inside ? cf[f] : 0.0f;
    }
}

// Where k_blend_contrib adds its per-Gaussian statistics and writes its id plane (nullable
// each), and the frame's overflow word (Stats::overflow).
struct ContribIO {
    uint32_t* count;
    unsigned long long* weight;
    uint32_t* wmax;
    int32_t* id;
    const uint32_t* overflow;
};

constexpr int kContribCount = 1, kContribWeight = 2, kContribMax = 4, kContribId = 8;

// Per-Gaussian contribution statistics and the id plane (gsr_render_contrib): k_blend_aux's
// schedule — one wave64 per 8x8 block, one-wave workgroups, the same block -> workgroup
// mapping and tile lists, the same 64-record batches, prefetch and conservative cull — and,
// for every survivor, the exact one-splat step (gsr_blend_md2, gsr_blend_expf, selects), so
// each pixel takes the decisions of render.cu:323-341.  No colours: a lane keeps its T, the
// largest weight w = fma(alpha, T, 0) it composited and that splat's Gaussian index.
//
// A scatter, not a composite: per survivor the wave reduces its taking lanes to one triple
// {popcount of the take ballot, sum of rint(w 2^24), max of w's float bits} (scalar values)
// and parks it in the survivor's RECORD lane, which still holds the Gaussian index in a
// register (saved before the prefetch overwrites cidx).  After the batch's loop every
// survivor lane with a non-zero count issues its own atomics: at most one per statistic per
// (wave, surviving splat), 64 distinct addresses per instruction, never one per pixel.  All
// three reductions are integer (the weights in fixed point: 64 values below 2^24 fit 32 bits
// in the wave, the global sum is 64-bit), so the totals do not depend on the order in which
// waves, frames or streams add to them.
//
// A frame whose overflow word is set (truncated tile lists or an incomplete depth order)
// returns at once: it adds nothing, and the caller renders it again.
//
// Survivor k's slot in the wave's LDS slice (8 dwords, read with wave-uniform addresses):
//   [0] cx [1] cy [2] a [3] b | [4] c [5] e [6] opacity [7] unused
// WHAT: the kContrib* bits of the outputs wanted; the others' reductions drop out.
template <int WHAT>
__global__ __launch_bounds__(64, 8) void k_blend_contrib(const uint32_t* __restrict__ idx,
                                                         const uint2* __restrict__ ranges,
                                                         const uint4* __restrict__ rec, int tiles_x, int tiles_y,
                                                         int W, int H, int cover_w, int cover_h, int bands,
                                                         ContribIO io) {
    constexpr bool CNT = (WHAT & kContribCount) != 0, WGT = (WHAT & kContribWeight) != 0;
    constexpr bool MAXW = (WHAT & kContribMax) != 0, ID = (WHAT & kContribId) != 0;
    constexpr bool STATS = CNT || WGT || MAXW;
    __shared__ float4 sP[64 * 2];
    if (*io.overflow) return;   // uniform: an incomplete frame adds nothing
    BlockSetup bs;
    if (!block_setup(bs, ranges, tiles_x, tiles_y, cover_w, cover_h, bands)) return;
    const uint32_t beg = bs.beg, end = bs.end;
    const int lane = bs.lane, px = bs.px, py = bs.py;
    const bool inside = bs.inside;
    const float fpx = bs.fpx, fpy = bs.fpy;
    const float4* wP4 = sP;

    // pixels outside the covered area start saturated and composite nothing (blend_block)
    float T = inside ? 1.0f : 0.0f;
    float best_w = 0.0f;
    int32_t best_i = -1;

    RecordBatch B;
    batch_first(B, idx, rec, beg, end, lane);
    bool alive = __ballot(!(T < 1e-3f)) != 0ull;
    for (uint32_t base = beg; base < end && alive; base += 64) {
        const uint32_t cnt = min(64u, end - base);
        // ---- cull (lane = record) ----
        BlockCull cl;
        const bool hit = block_cull(cl, B.ra, B.rc, B.rd, bs.bx, bs.by, lane, cnt, __ballot(!(T < 1e-3f)));
        const uint32_t dsc = cl.dsc;
        // ---- survivors, compacted in list order ----
        const uint64_t m = __ballot(hit);
        const uint32_t k_l = ballot_rank(m);
        if (hit) {
            float4* S4 = sP + k_l * 2;
            S4[0] = make_float4(__uint_as_float(B.rc.x), __uint_as_float(B.rc.y), __uint_as_float(B.ra.x),
                                __uint_as_float(B.ra.y));
            S4[1] = make_float4(__uint_as_float(B.ra.z), __uint_as_float(B.ra.w), __uint_as_float(B.rb.x), 0.0f);
        }
        const uint32_t gidx = B.cidx;   // this batch's Gaussian index of record `lane`
        batch_prefetch(B, idx, rec, base, end, lane);
        // ---- the exact one-splat step over the survivors (render.cu:329-340) ----
        uint32_t p_cnt = 0, p_sum = 0, p_max = 0;   // survivor `lane`'s reduced triple
        uint64_t mm = m;
        for (uint32_t k = 0; mm && alive; ++k) {
            const int s = __builtin_ctzll(mm);
            mm &= mm - 1;
            const uint64_t box = box_mask((uint32_t)__builtin_amdgcn_readlane((int)dsc, s));
            const float4 q0 = wP4[k * 2 + 0], q1 = wP4[k * 2 + 1];
            SplatStep st;
            const bool take = splat_step(st, fpx, fpy, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, box, T);
            const float alpha = st.alpha;
            const uint64_t tb = __ballot(take);
            if (tb) {   // uniform
                // the weight of the take: k_blend_aux's alpha channel step with ca = 0
                const float w = __builtin_fmaf(alpha, T, 0.0f);
                if (STATS) {
                    const bool mine = lane == s;
                    // (without the count output: 1 = composited at all, for the guard below)
                    const uint32_t pc = CNT ? (uint32_t)__builtin_popcountll(tb) : 1u;
                    p_cnt = mine ? pc : p_cnt;
                    if (WGT) {
                        const uint32_t fx = take ? __float2uint_rn(w * 16777216.0f) : 0u;
                        const uint32_t sum =
                            (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan(fx, OpAdd{}), 63);
                        p_sum = mine ? sum : p_sum;
                    }
                    if (MAXW) {
                        const uint32_t mx = wave_max_u32(take ? __float_as_uint(w) : 0u);
                        p_max = mine ? mx : p_max;
                    }
                }
                if (ID) {
                    const int32_t g = __builtin_amdgcn_readlane((int)gidx, s);
                    const bool better = take & (w > best_w);   // strictly: the first of equals stays
                    best_w = better ? w : best_w;
                    best_i = better ? g : best_i;
                }
                const float Tn = T * (1.0f - alpha);
                T = take ? Tn : T;
                alive = __ballot(!(T < 1e-3f)) != 0ull;
            }
        }
        // ---- one atomic per statistic per survivor that some pixel composited (lane = survivor) ----
        if (STATS && hit && p_cnt) {
            if (CNT) atomicAdd(io.count + gidx, p_cnt);
            if (WGT) atomicAdd(io.weight + gidx, (unsigned long long)p_sum);
            if (MAXW) atomicMax(io.wmax + gidx, p_max);
        }
    }
    if (ID && px < W && py < H) io.id[(size_t)py * (size_t)W + (size_t)px] = inside ? best_i : -1;
}

// The upstream gradients k_blend_backward reads (W*H planes, nullable each), the planar
// per-Gaussian gradient arrays it adds to (element [c * n + i], nullable each) and the
// frame's overflow word.
struct BackwardIO {
    const float* g_image;
    const float* g_alpha;
    float* color;
    float* opacity;
    float* conic;
    float* center;
    int64_t n;
    const uint32_t* overflow;
};

constexpr int kBackColor = 1, kBackOpacity = 2, kBackConic = 4, kBackCenter = 8;

// Sums of NV per-lane values over the wave, jointly: v_permlane32_swap folds two values into
// one register (lanes 0-31 then hold the first's sum over lane ^ 32, lanes 32-63 the
// second's), v_permlane16_swap folds two of those (even rows of 16 lanes the first, odd rows
// the second), and four row_ror adds finish inside the rows.  Afterwards every lane of row r
// holds in x[i] the wave's total of value backward_slot(i, r) (an odd tail is paired with
// itself, so some rows repeat a value): about NV / 2 + NV / 4 + NV adds (20 for nine values)
// against the 6 NV of separate scans.
template <int NV>
__device__ __forceinline__ void wave_sum_packed(const float (&v)[NV], float (&x)[(NV + 3) / 4]) {
    constexpr int NW = (NV + 1) / 2, NX = (NW + 1) / 2;
    float w[NW];
#pragma unroll
    for (int i = 0; i < NW; i++) {
        const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[2 * i]),
                                                        __float_as_uint(v[min(2 * i + 1, NV - 1)]), false, false);
        w[i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    }
#pragma unroll
    for (int i = 0; i < NX; i++) {
        const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(w[2 * i]),
                                                        __float_as_uint(w[min(2 * i + 1, NW - 1)]), false, false);
        float s = __uint_as_float(r[0]) + __uint_as_float(r[1]);
        s += __uint_as_float(dpp_u32<0x121, 0xf, true>(__float_as_uint(s)));   // row_ror:1
        s += __uint_as_float(dpp_u32<0x122, 0xf, true>(__float_as_uint(s)));   // row_ror:2
        s += __uint_as_float(dpp_u32<0x124, 0xf, true>(__float_as_uint(s)));   // row_ror:4
        s += __uint_as_float(dpp_u32<0x128, 0xf, true>(__float_as_uint(s)));   // row_ror:8
        x[i] = s;
    }
}
// Which of the NV values row r holds in x[i] after wave_sum_packed, or -1 for a repeat.
template <int NV>
__device__ __forceinline__ int backward_slot(int i, int r) {
    constexpr int NW = (NV + 1) / 2;
    const int wi = 2 * i + (r & 1), vi = 2 * wi + (r >> 1);
    return (wi < NW && vi < NV) ? vi : -1;
}

// The backward pass of the exact blend (gsr_render_backward): gradients of
// L = sum over pixels of g_rgb . image + g_A alpha with respect to every composited splat's
// record (colour, opacity, conic, centre), added to planar per-Gaussian arrays.
// k_blend_contrib's schedule and decisions — one wave64 per 8x8 block, one-wave workgroups,
// the same mapping, tile lists, 64-record batches, prefetch, conservative cull and survivor
// compaction, the exact one-splat step, the early return on the overflow word.
//
// Forward order, two sweeps of the block's list in one kernel.  With u_j = g_rgb . colour_j
// + g_A and P_j = sum_{k <= j} u_k alpha_k T_k, dL/dalpha_j = T_j u_j - (G - P_j) / (1 -
// alpha_j), G = P_last: sweep 0 accumulates only P and leaves G, sweep 1 runs the same
// instructions again (the sweep loop is not unrolled, so G - P_last is exactly 0) and forms
// the gradients.  No division of T, no reversed lists.
//
// Per survivor that some lane takes, the wanted components (colour 3, opacity 1, conic 3 —
// dL/db = dL/dc, one sum added to both planes — centre 2) are summed over the wave by
// wave_sum_packed and written over the survivor's own LDS slot, which the loop has finished
// reading; `taken` (a scalar mask) remembers which slots hold sums.  After the batch's loop
// each such survivor's record lane reads its sums back and issues the float atomics: one per
// component per (wave, taken splat), never one per pixel.  Their order of arrival is not
// fixed, so the totals are not reproducible in the last bits.
//
// Survivor k's slot (12 dwords, read with wave-uniform addresses):
//   [0] cx [1] cy [2] a [3] b | [4] c [5] e [6] opacity [7] r | [8] g [9] b [10..11] unused
// WHAT: the kBack* bits of the outputs wanted; the others' sums drop out.
template <int WHAT>
__global__ __launch_bounds__(64, 8) void k_blend_backward(const uint32_t* __restrict__ idx,
                                                          const uint2* __restrict__ ranges,
                                                          const uint4* __restrict__ rec, int tiles_x, int tiles_y,
                                                          int W, int H, int cover_w, int cover_h, int bands,
                                                          BackwardIO io) {
    constexpr bool COL = (WHAT & kBackColor) != 0, OPA = (WHAT & kBackOpacity) != 0;
    constexpr bool CON = (WHAT & kBackConic) != 0, CEN = (WHAT & kBackCenter) != 0;
    constexpr int oC = 0, oO = oC + (COL ? 3 : 0), oK = oO + (OPA ? 1 : 0), oX = oK + (CON ? 3 : 0);
    constexpr int NV = oX + (CEN ? 2 : 0), NX = (NV + 3) / 4;
    constexpr int kSlot = 12;
    __shared__ float4 sP[64 * (kSlot / 4)];
    if (*io.overflow) return;   // uniform: an incomplete frame adds nothing
    BlockSetup bs;
    if (!block_setup(bs, ranges, tiles_x, tiles_y, cover_w, cover_h, bands)) return;
    const uint32_t beg = bs.beg, end = bs.end;
    const int lane = bs.lane, px = bs.px, py = bs.py;
    const bool inside = bs.inside;
    const float fpx = bs.fpx, fpy = bs.fpy;
    const float4* wP4 = sP;
    float* wF = reinterpret_cast<float*>(sP);

    // the pixel's upstream gradient; pixels outside the covered area composite nothing
    float g_r = 0.0f, g_g = 0.0f, g_b = 0.0f, g_a = 0.0f;
    if (inside && px < W && py < H) {
        const size_t o = (size_t)py * (size_t)W + (size_t)px;
        const size_t hw = (size_t)W * (size_t)H;
        if (io.g_image) {
            g_r = io.g_image[o];
            g_g = io.g_image[hw + o];
            g_b = io.g_image[2 * hw + o];
        }
        if (io.g_alpha) g_a = io.g_alpha[o];
    }

    float G = 0.0f;
#pragma nounroll
    for (int sweep = 0; sweep < 2; ++sweep) {
        // pixels outside the covered area start saturated and composite nothing (blend_block)
        float T = inside ? 1.0f : 0.0f;
        float P = 0.0f;
        RecordBatch B;
        batch_first(B, idx, rec, beg, end, lane);
        bool alive = __ballot(!(T < 1e-3f)) != 0ull;
        for (uint32_t base = beg; base < end && alive; base += 64) {
            const uint32_t cnt = min(64u, end - base);
            // ---- cull (lane = record) ----
            BlockCull cl;
            const bool hit = block_cull(cl, B.ra, B.rc, B.rd, bs.bx, bs.by, lane, cnt, __ballot(!(T < 1e-3f)));
            const uint32_t dsc = cl.dsc;
            // ---- survivors, compacted in list order ----
            const uint64_t m = __ballot(hit);
            const uint32_t k_l = ballot_rank(m);
            if (hit) {
                float4* S4 = sP + k_l * (kSlot / 4);
                S4[0] = make_float4(__uint_as_float(B.rc.x), __uint_as_float(B.rc.y), __uint_as_float(B.ra.x),
                                    __uint_as_float(B.ra.y));
                S4[1] = make_float4(__uint_as_float(B.ra.z), __uint_as_float(B.ra.w), __uint_as_float(B.rb.x),
                                    __uint_as_float(B.rb.y));
                S4[2] = make_float4(__uint_as_float(B.rb.z), __uint_as_float(B.rb.w), 0.0f, 0.0f);
            }
            const uint32_t gidx = B.cidx;   // this batch's Gaussian index of record `lane`
            batch_prefetch(B, idx, rec, base, end, lane);
            // ---- the exact one-splat step over the survivors (render.cu:329-340) ----
            uint64_t taken = 0;   // survivors whose slot holds sums
            uint64_t mm = m;
            for (uint32_t k = 0; mm && alive; ++k) {
                const int s = __builtin_ctzll(mm);
                mm &= mm - 1;
                const uint64_t box = box_mask((uint32_t)__builtin_amdgcn_readlane((int)dsc, s));
                const float4 q0 = wP4[k * 3 + 0], q1 = wP4[k * 3 + 1], q2 = wP4[k * 3 + 2];
                SplatStep st;
                const bool take = splat_step(st, fpx, fpy, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, box, T);
                const float dx = st.dx, dy = st.dy, ee = st.ee, oe = st.oe, alpha = st.alpha;
                if (__ballot(take)) {   // uniform
                    const float u = __builtin_fmaf(g_r, q1.w, __builtin_fmaf(g_g, q2.x, __builtin_fmaf(g_b, q2.y, g_a)));
                    const float w = alpha * T;
                    const float Pn = __builtin_fmaf(u, w, P);
                    P = take ? Pn : P;
                    if (sweep) {
                        float v[NV];
                        const float wt = take ? w : 0.0f;
                        if (COL) {
                            v[oC % NV] = g_r * wt;
                            v[(oC + 1) % NV] = g_g * wt;
                            v[(oC + 2) % NV] = g_b * wt;
                        }
                        if (OPA || CON || CEN) {
                            // (1 - alpha >= 0.01; the clamped alpha passes nothing on)
                            float da = T * u - (G - P) * __builtin_amdgcn_rcpf(1.0f - alpha);
                            da = (take & !(oe > 0.99f)) ? da : 0.0f;
                            if (OPA) v[oO % NV] = da * ee;
                            const float dmd = -0.5f * oe * da;
                            if (CON) {
                                v[oK % NV] = dmd * dx * dx;
                                v[(oK + 1) % NV] = dmd * dx * dy;
                                v[(oK + 2) % NV] = dmd * dy * dy;
                            }
                            if (CEN) {
                                const float bc = q0.w + q1.x;
                                v[oX % NV] = -dmd * (2.0f * q0.z * dx + bc * dy);
                                v[(oX + 1) % NV] = -dmd * (bc * dx + 2.0f * q1.y * dy);
                            }
                        }
                        float x[NX];
                        wave_sum_packed<NV>(v, x);
                        if ((lane & 15) == 0) {
#pragma unroll
                            for (int i = 0; i < NX; i++) {
                                const int vi = backward_slot<NV>(i, lane >> 4);
                                if (vi >= 0) wF[k * kSlot + vi] = x[i];
                            }
                        }
                        taken |= 1ull << k;
                    }
                    const float Tn = T * (1.0f - alpha);
                    T = take ? Tn : T;
                    alive = __ballot(!(T < 1e-3f)) != 0ull;
                }
            }
            // ---- one atomic per component per survivor that some pixel composited (lane = survivor) ----
            if (sweep && hit && ((taken >> k_l) & 1ull)) {
                const float* r = wF + k_l * kSlot;
                const int64_t n = io.n;
                if (COL) {
                    atomicAdd(io.color + gidx, r[oC]);
                    atomicAdd(io.color + n + gidx, r[oC + 1]);
                    atomicAdd(io.color + 2 * n + gidx, r[oC + 2]);
                }
                if (OPA) atomicAdd(io.opacity + gidx, r[oO]);
                if (CON) {
                    atomicAdd(io.conic + gidx, r[oK]);
                    atomicAdd(io.conic + n + gidx, r[oK + 1]);
                    atomicAdd(io.conic + 2 * n + gidx, r[oK + 1]);
                    atomicAdd(io.conic + 3 * n + gidx, r[oK + 2]);
                }
                if (CEN) {
                    atomicAdd(io.center + gidx, r[oX]);
                    atomicAdd(io.center + n + gidx, r[oX + 1]);
                }
            }
        }
        G = P;
    }
}

// k_blend_backward_aux's upstream gradients (W*H planes, nullable each; g_feat: nfeat planes),
// the per-Gaussian values its depth and feature channels composite (as AuxIO), the planar
// per-Gaussian gradient arrays it adds to (nullable each) and the frame's overflow word.
struct BackwardAuxIO {
    const float* g_image;
    const float* g_alpha;
    const float* g_depth;
    const float* g_feat;
    const float* features;   // nfeat arrays of n floats (NF = 4, GEO)
    const float4* pack;      // k_aux_pack's output (NF = 8, GEO)
    const float* z;          // k_aux_depth's output (DEPTH, GEO)
    float* color;
    float* opacity;
    float* conic;
    float* center;
    float* dz;               // n floats
    float* feat;             // nfeat planes of n floats
    int64_t n;
    int nfeat;
    const uint32_t* overflow;
};

// The backward pass of the exact blend with the depth and feature channels
// (gsr_render_backward_aux): gradients of L = sum over pixels of g_rgb . image + g_A alpha +
// g_D depth + sum_f g_f feat_f.  k_blend_backward's schedule, decisions, two forward sweeps
// and in-wave reduction, with
//   u_j = g_rgb . colour_j + g_A + g_D z_j + sum_f g_f phi_f,j
// in place of its u, and two more linear outputs per taken splat: dz += g_D alpha T and
// feat[f] += g_f alpha T.  z and phi are gathered by Gaussian index by the hit lane, as
// k_blend_aux does it (up to four features from the planar arrays, more from k_aux_pack's
// interleaved copy), so they are the forward's floats.  Only u reads them: without GEO the
// slots' dwords [10] and [12 ..] hold nothing before the sums, and z, features and pack are
// not needed at all.
//
// Survivor k's slot (12 + NF dwords, read with wave-uniform addresses) is k_blend_aux's:
//   [0] cx [1] cy [2] a [3] b | [4] c [5] e [6] opacity [7] r | [8] g [9] b [10] -Z [11] unused
//   | [12 ..] features
// The sums go over the slot once the loop has read it: colour 3, then (GEO) opacity 1, conic
// 3, centre 2, then (DEPTH) z 1 from dword 0 on — at most 10 — and the feature sums in their
// own dwords from 12 on, reduced four at a time so that at most ten values are live at once.
//
// NF: the feature channels in u and in the sums, padded to 0 / 4 / 8.  DEPTH: g_D given (z in
// u, the z sum).  GEO: any of opacity, conic, centre wanted; without it nothing needs
// dL/dalpha, hence neither P nor G, and the kernel makes ONE sweep (every remaining output is
// linear in alpha T).  Which planes of a group are written is decided at the atomic.
// NF = 8 asks for six waves per SIMD like k_blend_aux<8> (5 KiB of LDS per wave), and so does
// NF = 4 with GEO, which at eight (64 VGPRs) spills 20 bytes.
template <int NF, bool DEPTH, bool GEO>
__global__ __launch_bounds__(64, (NF > 4 || (NF == 4 && GEO)) ? 6 : 8) void k_blend_backward_aux(
    const uint32_t* __restrict__ idx, const uint2* __restrict__ ranges, const uint4* __restrict__ rec, int tiles_x,
    int tiles_y, int W, int H, int cover_w, int cover_h, int bands, BackwardAuxIO io) {
    constexpr int oC = 0, oO = 3, oK = 4, oX = 7, oZ = GEO ? 9 : 3;
    constexpr int NV = oZ + (DEPTH ? 1 : 0), NX = (NV + 3) / 4;
    constexpr int kSlot = 12 + NF, oF = 12;
    constexpr int kNF = NF ? NF : 1;
    __shared__ float4 sP[64 * (kSlot / 4)];
    if (*io.overflow) return;   // uniform: an incomplete frame adds nothing
    BlockSetup bs;
    if (!block_setup(bs, ranges, tiles_x, tiles_y, cover_w, cover_h, bands)) return;
    const uint32_t beg = bs.beg, end = bs.end;
    const int lane = bs.lane, px = bs.px, py = bs.py;
    const bool inside = bs.inside;
    const float fpx = bs.fpx, fpy = bs.fpy;
    const float4* wP4 = sP;
    float* wF = reinterpret_cast<float*>(sP);

    // the pixel's upstream gradient; pixels outside the covered area composite nothing
    float g_r = 0.0f, g_g = 0.0f, g_b = 0.0f, g_a = 0.0f, g_d = 0.0f, g_f[kNF];
#pragma unroll
    for (int f = 0; f < kNF; f++) g_f[f] = 0.0f;
    if (inside && px < W && py < H) {
        const size_t o = (size_t)py * (size_t)W + (size_t)px;
        const size_t hw = (size_t)W * (size_t)H;
        if (io.g_image) {
            g_r = io.g_image[o];
            g_g = io.g_image[hw + o];
            g_b = io.g_image[2 * hw + o];
        }
        if (io.g_alpha) g_a = io.g_alpha[o];
        if (DEPTH) g_d = io.g_depth[o];
#pragma unroll
        for (int f = 0; f < NF; f++)   // padding channels: no upstream
            if (f < io.nfeat) g_f[f] = io.g_feat[(size_t)f * hw + o];
    }

    float G = 0.0f;
#pragma nounroll
    for (int sweep = GEO ? 0 : 1; sweep < 2; ++sweep) {
        // pixels outside the covered area start saturated and composite nothing (blend_block)
        float T = inside ? 1.0f : 0.0f;
        float P = 0.0f;
        RecordBatch B;
        batch_first(B, idx, rec, beg, end, lane);
        bool alive = __ballot(!(T < 1e-3f)) != 0ull;
        for (uint32_t base = beg; base < end && alive; base += 64) {
            const uint32_t cnt = min(64u, end - base);
            // ---- cull (lane = record) ----
            BlockCull cl;
            const bool hit = block_cull(cl, B.ra, B.rc, B.rd, bs.bx, bs.by, lane, cnt, __ballot(!(T < 1e-3f)));
            const uint32_t dsc = cl.dsc;
            // ---- survivors, compacted in list order; each gathers its -Z and features ----
            const uint64_t m = __ballot(hit);
            const uint32_t k_l = ballot_rank(m);
            const uint32_t gidx = B.cidx;   // this batch's Gaussian index of record `lane`
            float zv = 0.0f, fv[kNF];
#pragma unroll
            for (int f = 0; f < kNF; f++) fv[f] = 0.0f;
            if (hit) {
                // (only u reads -Z and the features: without GEO nothing gathers them)
                if (DEPTH && GEO) zv = io.z[gidx];
                if (GEO && NF == 8) {
                    const float4 p0 = io.pack[2 * (int64_t)gidx], p1 = io.pack[2 * (int64_t)gidx + 1];
                    fv[0] = p0.x; fv[1 % kNF] = p0.y; fv[2 % kNF] = p0.z; fv[3 % kNF] = p0.w;
                    fv[4 % kNF] = p1.x; fv[5 % kNF] = p1.y; fv[6 % kNF] = p1.z; fv[7 % kNF] = p1.w;
                } else if (GEO) {
#pragma unroll
                    for (int f = 0; f < NF; f++)   // padding channels repeat the last array (their g_f is 0)
                        fv[f] = io.features[(int64_t)min(f, io.nfeat - 1) * io.n + (int64_t)gidx];
                }
                float4* S4 = sP + k_l * (kSlot / 4);
                S4[0] = make_float4(__uint_as_float(B.rc.x), __uint_as_float(B.rc.y), __uint_as_float(B.ra.x),
                                    __uint_as_float(B.ra.y));
                S4[1] = make_float4(__uint_as_float(B.ra.z), __uint_as_float(B.ra.w), __uint_as_float(B.rb.x),
                                    __uint_as_float(B.rb.y));
            }
            const float col_g = __uint_as_float(B.rb.z), col_b = __uint_as_float(B.rb.w);
            batch_prefetch(B, idx, rec, base, end, lane);
            if (hit) {
                // (the gathered values last: their loads were issued ahead of the prefetch)
                float4* S4 = sP + k_l * (kSlot / 4);
                S4[2] = make_float4(col_g, col_b, zv, 0.0f);
                if (GEO && NF >= 4) S4[3] = make_float4(fv[0], fv[1 % kNF], fv[2 % kNF], fv[3 % kNF]);
                if (GEO && NF >= 8) S4[4] = make_float4(fv[4 % kNF], fv[5 % kNF], fv[6 % kNF], fv[7 % kNF]);
            }
            // ---- the exact one-splat step over the survivors (render.cu:329-340) ----
            uint64_t taken = 0;   // survivors whose slot holds sums
            uint64_t mm = m;
            for (uint32_t k = 0; mm && alive; ++k) {
                const int s = __builtin_ctzll(mm);
                mm &= mm - 1;
                const uint64_t box = box_mask((uint32_t)__builtin_amdgcn_readlane((int)dsc, s));
                const float4 q0 = wP4[k * (kSlot / 4) + 0], q1 = wP4[k * (kSlot / 4) + 1];
                const float4 q2 = wP4[k * (kSlot / 4) + 2];
                SplatStep st;
                const bool take = splat_step(st, fpx, fpy, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, box, T);
                const float dx = st.dx, dy = st.dy, ee = st.ee, oe = st.oe, alpha = st.alpha;
                if (__ballot(take)) {   // uniform
                    const float w = alpha * T;
                    float u = 0.0f;
                    if (GEO) {
                        u = __builtin_fmaf(g_r, q1.w, __builtin_fmaf(g_g, q2.x, __builtin_fmaf(g_b, q2.y, g_a)));
                        if (DEPTH) u = __builtin_fmaf(g_d, q2.z, u);
                        if (NF >= 4) {
                            const float4 q3 = wP4[k * (kSlot / 4) + 3];
                            u = __builtin_fmaf(g_f[0], q3.x, u);
                            u = __builtin_fmaf(g_f[1 % kNF], q3.y, u);
                            u = __builtin_fmaf(g_f[2 % kNF], q3.z, u);
                            u = __builtin_fmaf(g_f[3 % kNF], q3.w, u);
                        }
                        if (NF >= 8) {
                            const float4 q4 = wP4[k * (kSlot / 4) + 4];
                            u = __builtin_fmaf(g_f[4 % kNF], q4.x, u);
                            u = __builtin_fmaf(g_f[5 % kNF], q4.y, u);
                            u = __builtin_fmaf(g_f[6 % kNF], q4.z, u);
                            u = __builtin_fmaf(g_f[7 % kNF], q4.w, u);
                        }
                        const float Pn = __builtin_fmaf(u, w, P);
                        P = take ? Pn : P;
                    }
                    if (sweep) {
                        float v[NV];
                        const float wt = take ? w : 0.0f;
                        v[oC] = g_r * wt;
                        v[oC + 1] = g_g * wt;
                        v[oC + 2] = g_b * wt;
                        if (GEO) {
                            // (1 - alpha >= 0.01; the clamped alpha passes nothing on)
                            float da = T * u - (G - P) * __builtin_amdgcn_rcpf(1.0f - alpha);
                            da = (take & !(oe > 0.99f)) ? da : 0.0f;
                            v[oO % NV] = da * ee;
                            const float dmd = -0.5f * oe * da;
                            v[oK % NV] = dmd * dx * dx;
                            v[(oK + 1) % NV] = dmd * dx * dy;
                            v[(oK + 2) % NV] = dmd * dy * dy;
                            const float bc = q0.w + q1.x;
                            v[oX % NV] = -dmd * (2.0f * q0.z * dx + bc * dy);
                            v[(oX + 1) % NV] = -dmd * (bc * dx + 2.0f * q1.y * dy);
                        }
                        if (DEPTH) v[oZ % NV] = g_d * wt;
                        float x[NX];
                        wave_sum_packed<NV>(v, x);
                        if ((lane & 15) == 0) {
#pragma unroll
                            for (int i = 0; i < NX; i++) {
                                const int vi = backward_slot<NV>(i, lane >> 4);
                                if (vi >= 0) wF[k * kSlot + vi] = x[i];
                            }
                        }
#pragma unroll
                        for (int f0 = 0; f0 < NF; f0 += 4) {   // row r of the wave ends up with feature f0 + slot(0, r)
                            const float vf[4] = {g_f[f0 % kNF] * wt, g_f[(f0 + 1) % kNF] * wt, g_f[(f0 + 2) % kNF] * wt,
                                                 g_f[(f0 + 3) % kNF] * wt};
                            float xf[1];
                            wave_sum_packed<4>(vf, xf);
                            if ((lane & 15) == 0) wF[k * kSlot + oF + f0 + backward_slot<4>(0, lane >> 4)] = xf[0];
                        }
                        taken |= 1ull << k;
                    }
                    const float Tn = T * (1.0f - alpha);
                    T = take ? Tn : T;
                    alive = __ballot(!(T < 1e-3f)) != 0ull;
                }
            }
            // ---- one atomic per component per survivor that some pixel composited (lane = survivor) ----
            if (sweep && hit && ((taken >> k_l) & 1ull)) {
                const float* r = wF + k_l * kSlot;
                const int64_t n = io.n;
                if (io.color) {
                    atomicAdd(io.color + gidx, r[oC]);
                    atomicAdd(io.color + n + gidx, r[oC + 1]);
                    atomicAdd(io.color + 2 * n + gidx, r[oC + 2]);
                }
                if (GEO) {
                    if (io.opacity) atomicAdd(io.opacity + gidx, r[oO]);
                    if (io.conic) {
                        atomicAdd(io.conic + gidx, r[oK]);
                        atomicAdd(io.conic + n + gidx, r[oK + 1]);
                        atomicAdd(io.conic + 2 * n + gidx, r[oK + 1]);
                        atomicAdd(io.conic + 3 * n + gidx, r[oK + 2]);
                    }
                    if (io.center) {
                        atomicAdd(io.center + gidx, r[oX]);
                        atomicAdd(io.center + n + gidx, r[oX + 1]);
                    }
                }
                if (DEPTH && io.dz) atomicAdd(io.dz + gidx, r[oZ]);
                if (NF > 0 && io.feat) {
#pragma unroll
                    for (int f = 0; f < NF; f++)
                        if (f < io.nfeat) atomicAdd(io.feat + (int64_t)f * n + gidx, r[oF + f]);
                }
            }
        }
        G = P;
    }
}

}  // namespace

// ------------------------------------------------------------------ launchers

hipError_t launch_aux_depth(const float* arrays, int64_t stride, int64_t n, const Frame& fr, bool four_d, float t,
                            float* z, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const dim3 g(grid_for(n, 256));
    if (four_d) hipLaunchKernelGGL((k_aux_depth<true>), g, dim3(256), 0, s, arrays, stride, n, fr, t, z);
    else hipLaunchKernelGGL((k_aux_depth<false>), g, dim3(256), 0, s, arrays, stride, n, fr, t, z);
    return hipGetLastError();
}

hipError_t launch_blend_aux(const uint32_t* idx, const uint2* ranges, const uint4* rec, const Frame& fr,
                            float* out, float* alpha, float* depth, const float* z, const float* features,
                            int64_t n, int nfeat, float* feat_out, float4* pack, int band_tiles,
                            hipStream_t s) {
    if (nfeat < 0 || nfeat > 8 || (nfeat > 0 && (!features || !feat_out)) || (depth && n > 0 && !z) ||
        (nfeat > 4 && n > 0 && !pack) ||
        (!out && !alpha && !depth && nfeat == 0))
        return hipErrorInvalidValue;
    const int nt = fr.tiles_x * fr.tiles_y;
    if (nt <= 0) return hipSuccess;
    int bands, ng;
    blend_grid(nt, band_tiles, bands, ng);
    if (nfeat > 4 && n > 0)
        hipLaunchKernelGGL(k_aux_pack, dim3(grid_for(n, 256)), dim3(256), 0, s, features, n, nfeat, pack);
    const AuxIO io{out, alpha, depth, feat_out, features, pack, depth ? z : nullptr, n, nfeat};
    // features padded to 0 / 4 / 8 channels
    auto go = [&](auto nf) {
        constexpr int NF = decltype(nf)::value;
        with_bool(out != nullptr, [&](auto color) {
            hipLaunchKernelGGL((k_blend_aux<NF, decltype(color)::value>), dim3(ng), dim3(64), 0, s, idx, ranges, rec,
                               fr.tiles_x, fr.tiles_y, fr.W, fr.H, fr.cover_w, fr.cover_h, bands, io);
        });
    };
    if (nfeat == 0) go(std::integral_constant<int, 0>{});
    else if (nfeat <= 4) go(std::integral_constant<int, 4>{});
    else go(std::integral_constant<int, 8>{});
    return hipGetLastError();
}

hipError_t launch_blend_contrib(const uint32_t* idx, const uint2* ranges, const uint4* rec, const Frame& fr,
                                uint32_t* count, unsigned long long* weight, uint32_t* wmax, int32_t* id,
                                const uint32_t* overflow, int band_tiles, hipStream_t s) {
    const int what = (count ? kContribCount : 0) | (weight ? kContribWeight : 0) | (wmax ? kContribMax : 0) |
                     (id ? kContribId : 0);
    if (!what || !overflow) return hipErrorInvalidValue;
    const int nt = fr.tiles_x * fr.tiles_y;
    if (nt <= 0) return hipSuccess;
    int bands, ng;
    blend_grid(nt, band_tiles, bands, ng);
    const ContribIO io{count, weight, wmax, id, overflow};
    with_int_1_15(what, [&](auto w) {
        hipLaunchKernelGGL((k_blend_contrib<decltype(w)::value>), dim3(ng), dim3(64), 0, s, idx, ranges, rec,
                           fr.tiles_x, fr.tiles_y, fr.W, fr.H, fr.cover_w, fr.cover_h, bands, io);
    });
    return hipGetLastError();
}

hipError_t launch_blend_backward(const uint32_t* idx, const uint2* ranges, const uint4* rec, const Frame& fr,
                                 const float* g_image, const float* g_alpha, float* color, float* opacity,
                                 float* conic, float* center, int64_t n, const uint32_t* overflow, int band_tiles,
                                 hipStream_t s) {
    const int what = (color ? kBackColor : 0) | (opacity ? kBackOpacity : 0) | (conic ? kBackConic : 0) |
                     (center ? kBackCenter : 0);
    if (!what || (!g_image && !g_alpha) || !overflow) return hipErrorInvalidValue;
    const int nt = fr.tiles_x * fr.tiles_y;
    if (nt <= 0 || n <= 0) return hipSuccess;
    int bands, ng;
    blend_grid(nt, band_tiles, bands, ng);
    const BackwardIO io{g_image, g_alpha, color, opacity, conic, center, n, overflow};
    with_int_1_15(what, [&](auto w) {
        hipLaunchKernelGGL((k_blend_backward<decltype(w)::value>), dim3(ng), dim3(64), 0, s, idx, ranges, rec,
                           fr.tiles_x, fr.tiles_y, fr.W, fr.H, fr.cover_w, fr.cover_h, bands, io);
    });
    return hipGetLastError();
}

hipError_t launch_blend_backward_aux(const uint32_t* idx, const uint2* ranges, const uint4* rec, const Frame& fr,
                                     const float* g_image, const float* g_alpha, const float* g_depth,
                                     const float* g_feat, const float* features, int nfeat, const float* z,
                                     float4* pack, float* color, float* opacity, float* conic, float* center,
                                     float* dz, float* feat, int64_t n, const uint32_t* overflow, int band_tiles,
                                     hipStream_t s) {
    if (nfeat < 0 || nfeat > 8 || (nfeat > 0 && !features) || (nfeat == 0 && (g_feat || feat)) ||
        (!g_image && !g_alpha && !g_depth && !g_feat) ||
        (!color && !opacity && !conic && !center && !dz && !feat) || !overflow)
        return hipErrorInvalidValue;
    // an output whose upstream is missing is identically zero: not touched
    if (!g_image) color = nullptr;
    if (!g_depth) dz = nullptr;
    if (!g_feat) feat = nullptr;
    const bool geo = opacity || conic || center;
    if (!geo && !color && !dz && !feat) return hipSuccess;
    // what the kernel has to carry: the depth and feature channels only where they reach an output
    const bool depth = g_depth && (geo || dz);
    const int nf = (g_feat && (geo || feat)) ? nfeat : 0;
    if (!depth && nf == 0)   // nothing beyond k_blend_backward's function
        return launch_blend_backward(idx, ranges, rec, fr, g_image, g_alpha, color, opacity, conic, center, n, overflow,
                                     band_tiles, s);
    // (-Z and the feature values enter through u alone, which only the geometry outputs need)
    if (geo && ((depth && !z) || (nf > 4 && !pack))) return hipErrorInvalidValue;
    const int nt = fr.tiles_x * fr.tiles_y;
    if (nt <= 0 || n <= 0) return hipSuccess;
    int bands, ng;
    blend_grid(nt, band_tiles, bands, ng);
    if (geo && nf > 4) hipLaunchKernelGGL(k_aux_pack, dim3(grid_for(n, 256)), dim3(256), 0, s, features, n, nf, pack);
    const BackwardAuxIO io{g_image, g_alpha, depth ? g_depth : nullptr, nf ? g_feat : nullptr, features, pack,
                           (depth && geo) ? z : nullptr, color, opacity, conic, center, dz, nf ? feat : nullptr, n, nf,
                           overflow};
    // features padded to 0 / 4 / 8 channels
    auto go = [&](auto nfc) {
        constexpr int NF = decltype(nfc)::value;
        with_bool(depth, [&](auto d) {
            with_bool(geo, [&](auto g) {
                // (NF = 0 without DEPTH went to launch_blend_backward above: not instantiated)
                if constexpr (NF > 0 || decltype(d)::value)
                    hipLaunchKernelGGL((k_blend_backward_aux<NF, decltype(d)::value, decltype(g)::value>), dim3(ng),
                                       dim3(64), 0, s, idx, ranges, rec, fr.tiles_x, fr.tiles_y, fr.W, fr.H,
                                       fr.cover_w, fr.cover_h, bands, io);
            });
        });
    };
    if (nf == 0) go(std::integral_constant<int, 0>{});
    else if (nf <= 4) go(std::integral_constant<int, 4>{});
    else go(std::integral_constant<int, 8>{});
    return hipGetLastError();
}

}  // namespace gsr

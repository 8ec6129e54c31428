// gsr_blend.hip — the blend stage of the gfx950 (CDNA4) 3DGS rasterizer: k_blend_w (exact,
// fast-exp and depth-split blends, diagnostics and timeline variants), its exp functions and
// the probe that checks them exhaustively (DESIGN.md sections 3 and 9).
//
// Every float expression restates render.cu in the same operation order; the file is
// compiled with -ffp-contract=off so no FMA is formed implicitly, and the transcendental
// functions come from gsr_detmath.h, so the results are bit-identical to the CPU oracle
// (oracle/gsr_oracle.c).  The block walk shared with the derived passes
// (gsr_blend_derived.hip): gsr_blend_device.h.
#include "gsr_blend_device.h"

namespace gsr {

namespace {

typedef float f2 __attribute__((ext_vector_type(2)));

// Packed product with the HIGH half of the second operand broadcast to both lanes,
// in one v_pk_mul_f32 through op_sel (the compiler otherwise copies that half into
// a fresh register pair first: one v_mov per use in the compositing loop).
// Same IEEE products as the plain expressions (multiplication commutes exactly).
__device__ __forceinline__ f2 pk_mul_b_hi(f2 a, f2 b) {   // (a.x * b.y, a.y * b.y)
    f2 r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// Packed fused multiply-adds with the second factor's LOW / HIGH half broadcast:
// (fma(a.x, b.x, c.x), fma(a.y, b.x, c.y)) and (fma(a.x, b.y, c.x), fma(a.y, b.y, c.y)).
__device__ __forceinline__ f2 pk_fma_b_lo(f2 a, f2 b, f2 c) {
    f2 r;
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[1,0,1]" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ f2 pk_fma_b_hi(f2 a, f2 b, f2 c) {
    f2 r;
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// gsr_blend_expf on two lanes at once (v_pk_* for every float op that has a packed
// form: 11 packed + 4 single VALU, against 11 + 6 for the Cephes gsr_expf), for
// inputs the caller has PROVEN finite and in [-2e7, 5]: on [-104, 5] the clamp and
// the NaN select do not change the result and every remaining step is the same IEEE
// operation in the same order, so each half is bit-identical to gsr_blend_expf of
// that half.  Below -104 (no clamp here) n <= -150 — for |x log2 e| >= 2^22 the
// shifter no longer rounds to an integer and the remainder r drifts to |r| < 1.5,
// still finite — so ldexp(y, n) rounds to +0, the clamped result
// (gsr_exp_probe counts the halves that differ from the scalar function over every
// float of [-2e7, 5]: none).  Out-of-box lanes are discarded by the caller.
__device__ __forceinline__ f2 gsr_blend_expf_x2(f2 xc) {
    const f2 t = __builtin_elementwise_fma(xc, (f2)1.44269504088896341f, (f2)12582912.0f);
    const f2 n = t - 12582912.0f;
    f2 r = __builtin_elementwise_fma(-n, (f2)0.693359375f, xc);
    r = __builtin_elementwise_fma(-n, (f2)-2.12194440e-4f, r);
    f2 q = __builtin_elementwise_fma((f2)0x1.6b42a4p-10f, r, (f2)0x1.125e6cp-7f);
    q = __builtin_elementwise_fma(q, r, (f2)0x1.5557c2p-5f);
    q = __builtin_elementwise_fma(q, r, (f2)0x1.555452p-3f);
    q = __builtin_elementwise_fma(q, r, (f2)0x1.fffffcp-2f);
    const f2 r2 = r * r;
    const f2 y = __builtin_elementwise_fma(q, r2, r) + 1.0f;
    f2 res;
    res.x = __builtin_amdgcn_ldexpf(y.x, (int)n.x);
    res.y = __builtin_amdgcn_ldexpf(y.y, (int)n.y);
    return res;
}

// The blend's fast exp (GSR_TUNE_BLEND_EXP 1): e^x as the hardware 2^t (v_exp_f32) of
// t = x log2(e), two lanes at once.  Its relative difference from gsr_blend_expf, with the
// alpha product, is bounded on the argument range a composited lane can have
// (kFxEpsMax, kFxEpsBig below; measured exhaustively by gsr_exp_probe); the
// alpha decisions never use it (xs), and the transmittance test is guarded.
__device__ __forceinline__ f2 fast_expf_x2(f2 x) {
    const f2 t = x * 1.44269504088896341f;
    f2 q;
    q.x = __builtin_amdgcn_exp2f(t.x);
    q.y = __builtin_amdgcn_exp2f(t.y);
    return q;
}

// Fast-exp blend: bounds on |alpha_fast / alpha_exact - 1| for a composited lane
// (opacity in [0, 1] and alpha_exact >= 1e-3, so the exp argument x lies in
// [ln(1e-3), 5]; alpha > 0.5 needs x > ln 0.5, alpha > 0.9 needs x > ln 0.9).  Each is
// the exhaustive maximum of |fast_expf / gsr_blend_expf - 1| over every float x of its
// range (gsr_exp_probe; tests/test_gpu_fastexp.py checks these constants stay above
// it) plus 2^-23 for the two roundings of op * e:
//   kFxEps3  all composited lanes (x >= -6.95)
//   kFxEps2  alpha > 0.5            (x >= -0.70)
//   kFxEps1  alpha > 0.9            (x >= -0.11)
// The transmittance of a pixel then differs from the exact chain's by a relative
//   rho <= 207.1 kFxEps1 + 6.9078 max(3.909 kFxEps2, 1.4427 kFxEps3) + 3 2^-24 n
// (n = composited splats, bounded by the wave's splat-iterations) up to and including
// the step where it first drops below 1e-3 ("Fast exp"):
// kFxBand0 and kFxBandStep are those terms with 2 % headroom.  The n term counts the
// roundings per composite: the exact chain's two (1 - alpha, then the product) and the
// fast chain's one (T - T alpha as one fma).
constexpr float kFxEps3 = 6.6e-7f;
constexpr float kFxEps2 = 4.8e-7f;
constexpr float kFxEps1 = 4.8e-7f;
constexpr float kFxBand0 = 1.02f * (207.1f * kFxEps1 + 6.9078f * (3.909f * kFxEps2 > 1.4427f * kFxEps3
                                                                  ? 3.909f * kFxEps2 : 1.4427f * kFxEps3));
constexpr float kFxBandStep = 1.02f * 3.0f * 0x1p-24f;

// Set in the batch's last pair's second box descriptor (bit 30: above the survivor lane
// at bits 24-29; box_mask reads bits 0-21 only).
constexpr uint32_t kLastPair = 0x40000000u;

// n + (lane's bit of ma) + (lane's bit of mb): the wave masks are the carry-ins of two
// v_addc_co_u32 (one VALU each; counting booleans compiles to selects and an add).
__device__ __forceinline__ uint32_t count_lanes2(uint32_t n, uint64_t ma, uint64_t mb) {
    uint64_t c0, c1;
    asm("v_addc_co_u32_e64 %0, %1, %2, 0, %3" : "=v"(n), "=s"(c0) : "v"(n), "s"(ma));
    asm("v_addc_co_u32_e64 %0, %1, %2, 0, %3" : "=v"(n), "=s"(c1) : "v"(n), "s"(mb));
    (void)c0;
    (void)c1;
    return n;
}

// The band for one pixel from what it composited so far: n splats, the largest alpha
// m.  Besides the worst case above (band0 = kFxBand0), the alpha terms obey
//   sum alpha_i / (1 - alpha_i) <= (sum alpha_i) / (1 - m)
//                              <= (ln 1000 + ln(1 / (1 - m))) / (1 - m)
// (alpha <= -ln(1 - alpha), and the exact T stayed >= 1e-3 before the step being
// tested, whose own alpha is <= m), so rho <= kFxEps3 of that, which is far smaller
// unless some alpha came near 0.99.  2 % headroom over the hardware log / rcp.
// band0 < 0 (measurement builds only) turns the guard off.
__device__ __forceinline__ float fx_band(float band0, uint32_t n, float m) {
    const float om = 1.0f - m;                                 // >= 0.01 (alpha <= 0.99)
    const float lnm = -0.693147181f * __builtin_amdgcn_logf(om);   // ln(1 / (1 - m))
    const float byM = 1.02f * kFxEps3 * (6.9078f + lnm) * __builtin_amdgcn_rcpf(om);
    return __builtin_fmaf((float)n, kFxBandStep, band0 < 0.0f || band0 > 0.5f ? band0 : fminf(band0, byM));
}

// One wave64 per 8x8 pixel block (four per 16x16 tile, one tile per
// workgroup), no workgroup barrier.  Each wave streams its tile's splat list in
// 64-record batches (records of batch k+1 and indices of batch k+2 prefetched
// into registers).  Per batch, lane l culls record l (AABB, then the exact
// ellipse-vs-block test) and computes its 64-bit in-AABB pixel mask; the
// survivors are compacted, in list order, into PAIR SLOTS of the wave's LDS
// slice so that {parameter of splat 2j, parameter of splat 2j+1} are adjacent
// and feed v_pk_* instructions directly.  The compositing loop takes two
// splats per iteration: md2, exp and alpha packed, then the two composites in
// list order.  Batches holding a survivor without the fast-path proof run an
// exact one-splat path instead (same values, full gsr_blend_expf, plain selects).
//
// Pair slot dwords (h = 0 / 1 for the first / second splat of the pair):
//   [0+h] cx  [2+h] cy  [4+h] a  [6+h] b  [8+h] c  [10+h] e  [12+h] opacity
//   [14+2h] red  [15+2h] green  [18+h] blue  (fast exp only: [20+h] xs)
//   [22+h] box descriptor | survivor lane << 24 (0: no splat)
struct BlendDiag {
    uint64_t loaded = 0, iter = 0, active = 0, taken = 0, slow = 0, zero_taken = 0, no_cand_pairs = 0;
};

// Diagnostics take map: per pixel, the number of splats composited and a sum of
// a mix of their Gaussian indices (the oracle's orc_render_takes computes the same).
__device__ __forceinline__ uint32_t take_mix(uint32_t g) { return (g + 1u) * 2654435761u; }

// Depth split: the next frame's threshold from this frame's near depth order: the key
// at position na (the host's split point) when the near part holds more than na items,
// else the threshold widened in proportion from the smallest key.  Any threshold gives
// the same image.
__device__ __forceinline__ void split_cut_update(const SplitCut& sc) {
    const uint64_t* sorted = depth_sorted(sc.items0, sc.items1, sc.dstats);
    const uint32_t m = sc.nnear ? min(*sc.nnear, sc.n) : sc.n;
    uint32_t K;
    if (sc.na < m) {
        K = (uint32_t)(sorted[sc.na] >> 32);
    } else {
        const uint32_t k0 = *sc.kcut, kmin = m ? (uint32_t)(sorted[0] >> 32) : 0u;
        if (m == 0 || k0 == 0xffffffffu || k0 <= kmin) {
            K = 0xffffffffu;
        } else {
            const uint64_t span = (uint64_t)(k0 - kmin) * sc.na / m + 1u;
            K = (uint32_t)min((uint64_t)kmin + span, (uint64_t)0xffffffffu);
        }
    }
    *sc.kcut = K;
}

// One 8x8 pixel block (bx, by) blended by one wave over the tile list
// idx[beg, end), using the wave's private LDS slice wP (32 pair slots).
//
// FX (fast exp, GSR_TUNE_BLEND_EXP 1): alpha from fast_expf_x2; the alpha test is
// the exact one through the record's xs (-md2/2 >= xs, gsr_alpha_take_min_x), so
// only the transmittance can differ from the exact chain, by less than the band
// kFxBand0 + kFxBandStep n.  The wave flags a pixel ("suspect") when a value of T on
// either side of its first drop below 1e-3 lies within the band of 1e-3, or when
// it ends unsaturated within the band; then the exact T could have taken the other
// branch.  The block writes every other pixel and returns the suspect mask; the
// caller blends the suspect pixels again exactly (FX false, `only` = the mask).  A
// batch holding a record without the fast proof aborts the fast pass (all ones, no
// pixel written).  Every pixel therefore composites exactly the splats the exact
// blend composites, in the same order.
//
// SPLIT (depth split, exact blend only): 1 = phase A, which composites the block's
// phase-A list and, when some pixel is still unsaturated at its end, saves every
// pixel's T in tsave (64 floats), sets *flag and counts the block in *gate (else
// clears *flag); 2 = phase B, which resumes such a block from the saved T and the
// colours phase A wrote (and, with DIAG, the take map).  Each pixel composites the
// same splats in the same order as over the whole list (the phase-A list is the
// nearest part of it, the phase-B list the rest), with the same operations.
template <bool DIAG, bool FX, int SPLIT>
__device__ __forceinline__ uint64_t blend_block(const uint32_t* __restrict__ idx, const uint4* __restrict__ rec,
                                                uint32_t beg, uint32_t end, int bx, int by, int lane, int W,
                                                int H, int cover_w, int cover_h, float* __restrict__ out,
                                                float* wP, BlendDiag& dg, uint64_t* __restrict__ tmap,
                                                float band0, uint64_t only, float* __restrict__ tsave = nullptr,
                                                uint8_t* __restrict__ flag = nullptr,
                                                uint32_t* __restrict__ gate = nullptr) {
    static_assert(SPLIT == 0 || !FX, "the depth split runs the exact blend");
    constexpr int kSlot = 24;                               // dwords per pair slot
    const int px = bx + (lane & 7), py = by + (lane >> 3);
    const bool inside = px < cover_w && py < cover_h;
    const float fpx = (float)px, fpy = (float)py;
    // transmittance; a pixel is saturated ("done", render.cu:328) iff T < 1e-3.
    // Pixels outside the covered area start saturated (T = 0) and write 0; so do the
    // pixels outside `only` (the exact re-blend of a fast block's suspect pixels).
    const bool mine = ((only >> lane) & 1ull) != 0ull;
    float T = inside && mine ? 1.0f : 0.0f;
    f2 crg = (f2)0.0f;
    float cb = 0.0f;
    const float4* wP4 = reinterpret_cast<const float4*>(wP);
    uint64_t suspect = 0;      // FX: pixels whose T decisions the band cannot vouch for
    uint32_t ntk = 0;          // FX: splats this pixel composited so far
    float amax = 0.0f;         // FX: largest alpha it composited
    float tprev = 1.0f;        // FX: T before the pixel's latest composite
    uint32_t tcount = 0, thash = 0;   // DIAG take map
    if (SPLIT == 2 && inside) {
        // inside => px < W and py < H (cover_w <= W, cover_h <= H)
        const size_t o = (size_t)py * (size_t)W + (size_t)px, hw = (size_t)W * (size_t)H;
        T = tsave[lane];
        crg.x = out[o];
        crg.y = out[hw + o];
        cb = out[2 * hw + o];
        if (DIAG && tmap) {
            const uint64_t tm = tmap[o];
            tcount = (uint32_t)tm;
            thash = (uint32_t)(tm >> 32);
        }
    }

    // the record batch (RecordBatch) in plain locals, loaded and prefetched here as batch_first
    // and batch_prefetch do it for the derived passes: behind those two functions the fast-exp
    // instantiation spills (gsr_blend_device.h)
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
        // ---- cull + lane masks + compaction (lane = record) ----
        BlockCull cl;
        const bool hit = block_cull(cl, ra, rc, rd, bx, by, lane, cnt, __ballot(!(T < 1e-3f)));
        const uint32_t dsc = cl.dsc;
        bool fast = cl.SMM <= 4e7f;   // per-block part of the fast-path proof
        // the fast exp's error bound assumes opacity in [0, 1] (NaN fails)
        if (FX) fast = fast && __uint_as_float(rb.x) <= 1.0f;
        const uint64_t m = __ballot(hit);
        const uint32_t nsurv = (uint32_t)__popcll(m);
        const bool all_fast = __ballot(hit & !fast) == 0ull;
        if (FX && !all_fast) return ~0ull;   // exact re-blend of the whole block
        if (hit) {
            const uint32_t k = ballot_rank(m);
            float* S = wP + (k >> 1) * kSlot;
            const int h = (int)(k & 1u);
            S[0 + h] = __uint_as_float(rc.x);
            S[2 + h] = __uint_as_float(rc.y);
            // fast batches store the conic pre-scaled by -0.5 (exact, see coef_ok)
            const float sc = all_fast ? -0.5f : 1.0f;
            S[4 + h] = sc * __uint_as_float(ra.x);
            S[6 + h] = sc * __uint_as_float(ra.y);
            S[8 + h] = sc * __uint_as_float(ra.z);
            S[10 + h] = sc * __uint_as_float(ra.w);
            S[12 + h] = __uint_as_float(rb.x);
            S[14 + 2 * h] = __uint_as_float(rb.y);
            S[15 + 2 * h] = __uint_as_float(rb.z);
            S[18 + h] = __uint_as_float(rb.w);
            if (FX) S[20 + h] = __uint_as_float(rd.x);
            // box descriptor (box_mask) | survivor lane << 24: the compositing loop reads
            // both splats' from the slot instead of walking the survivor mask.  The last
            // pair's second descriptor carries kLastPair (below)
            S[22 + h] = __uint_as_float(dsc | ((uint32_t)lane << 24) | (k + 1u == nsurv && h ? kLastPair : 0u));
        }
        if ((nsurv & 1u) && lane < 11) {
            // odd count: zero the unused second half of the last slot (descriptor 0 = empty
            // box keeps it inert); second-half dwords of a slot: 1 3 5 7 9 11 13 | 16 17 |
            // 19 | 23 (arithmetic, not a table: a table load would stall the wave on memory
            // once per odd batch)
            // (dword 23, the pair's second descriptor: kLastPair alone, an empty box)
            wP[(nsurv >> 1) * kSlot + (lane < 7 ? 2 * lane + 1 : lane < 10 ? lane + 9 + (lane == 9) : 23)] =
                lane == 10 ? __uint_as_float(kLastPair) : 0.0f;
        }
        if (DIAG) dg.loaded += cnt;
        const float xs_l = DIAG ? __uint_as_float(rd.x) : 0.0f;   // diagnostics: xs of record `lane`
        const uint32_t gi_l = cidx;                                // diagnostics: its Gaussian index
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

        uint64_t mm = m;
        if (all_fast) {
            // lanes not yet saturated; the end-of-iteration ballot of T2 is the next
            // iteration's "!(T < 1e-3)" (render.cu:328), so it is compared once
            uint64_t live = __ballot(!(T < 1e-3f));
            f2 TT;
            TT.x = T;
            TT.y = T;
            const uint32_t npairs = (uint32_t)__builtin_amdgcn_readfirstlane((int)((nsurv + 1u) >> 1));
            // one exit test per pair: after the batch's last pair `live` is 0 (the threshold
            // above; the next batch recomputes it from T), so the loop stops when the block
            // saturates or the batch ends
            if (npairs != 0u) {
#pragma unroll
            for (uint32_t j = 0; j < 32u;) {   // unrolled: the slot offsets are immediates
                const float4 q0 = wP4[j * (kSlot / 4) + 0], q1 = wP4[j * (kSlot / 4) + 1];
                const float4 q2 = wP4[j * (kSlot / 4) + 2], q3 = wP4[j * (kSlot / 4) + 3];
                const float4 q4 = wP4[j * (kSlot / 4) + 4];
                // the pair's box descriptors from the slot (one v_readfirstlane each); the
                // 64-bit lane masks are rebuilt from them by scalar instructions.  The
                // unused half of an odd batch's last slot holds descriptor 0: an empty box.
                // No survivor-mask walk, no "second splat?" selects: the loop's scalar
                // work is a co-bound of the VALU work (round 4).
                uint32_t dd0, dd1;
                float2 xs;
                if (FX) {
                    const float4 q5 = wP4[j * (kSlot / 4) + 5];
                    xs = make_float2(q5.x, q5.y);
                    dd0 = __float_as_uint(q5.z);
                    dd1 = __float_as_uint(q5.w);
                } else {
                    const float2 dd = *reinterpret_cast<const float2*>(wP + j * kSlot + 22);
                    dd0 = __float_as_uint(dd.x);
                    dd1 = __float_as_uint(dd.y);
                }
                const uint32_t d0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)dd0);
                const uint32_t d1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)dd1);
                const uint64_t box0 = box_mask(d0), box1 = box_mask(d1);
                const bool has1 = (d1 & 0xffu) != 0u;                        // diagnostics
                const int s0 = (int)(d0 >> 24), s1 = has1 ? (int)((d1 >> 24) & 63u) : s0;
                // render.cu:329-332, same operation order and fused multiply-adds
                // (gsr_blend_md2), both splats at once; the conic is stored pre-scaled
                // by -0.5, so this is -0.5f * md2 exactly
                const f2 dx = (f2)fpx - (f2){q0.x, q0.y};
                const f2 dy = (f2)fpy - (f2){q0.z, q0.w};
                const f2 u = __builtin_elementwise_fma((f2){q1.x, q1.y}, dx, (f2){q1.z, q1.w} * dy);
                const f2 v = __builtin_elementwise_fma((f2){q2.x, q2.y}, dx, (f2){q2.z, q2.w} * dy);
                const f2 mdh = __builtin_elementwise_fma(dx, u, dy * v);
                const f2 ee = FX ? fast_expf_x2(mdh) : gsr_blend_expf_x2(mdh);
                const f2 al = (f2){q3.x, q3.y} * ee;
                const float al0 = fminf(al.x, 0.99f), al1 = fminf(al.y, 0.99f);
                // alpha tests (render.cu:335): on alpha itself, or (FX) on the exp
                // argument against xs — the same decisions
                bool pass0, pass1;
                if (FX) {
                    pass0 = !(mdh.x < xs.x);
                    pass1 = !(mdh.y < xs.y);
                } else {
                    pass0 = !(al0 < 1e-3f);
                    pass1 = !(al1 < 1e-3f);
                }
                // render.cu:333-340: splat 2j, then splat 2j+1 against what 2j left
                const bool in0 = __builtin_amdgcn_inverse_ballot_w64(box0 & live);
                const bool in1 = __builtin_amdgcn_inverse_ballot_w64(box1);
                // (a0, a1) and (T, T1) live in register pairs, written in place, so
                // the packed blue product needs no moves; TT.x carries T across.
                // FX forms the take decisions as wave masks (the composited-splat
                // count below uses them as carry-ins)
                uint64_t t0m = 0, t1m = 0;
                bool take0, take1;
                f2 AA;
                if (FX) {
                    t0m = box0 & live & __builtin_amdgcn_ballot_w64(pass0);
                    take0 = __builtin_amdgcn_inverse_ballot_w64(t0m);
                    tprev = take0 ? TT.x : tprev;
                } else {
                    take0 = in0 & pass0;
                }
                AA.x = take0 ? al0 : 0.0f;
                // T (1 - alpha) (render.cu:339); the fast blend folds it into one fma, T - T alpha
                // with one rounding (kFxBandStep: 3 2^-24 per composite, 1 here and 2 in the
                // exact chain)
                TT.y = FX ? __builtin_fmaf(-TT.x, AA.x, TT.x) : TT.x * (1.0f - AA.x);
                if (FX) {
                    t1m = box1 & __builtin_amdgcn_ballot_w64(!(TT.y < 1e-3f)) & __builtin_amdgcn_ballot_w64(pass1);
                    take1 = __builtin_amdgcn_inverse_ballot_w64(t1m);
                    tprev = take1 ? TT.y : tprev;
                } else {
                    take1 = in1 & !(TT.y < 1e-3f) & pass1;
                }
                AA.y = take1 ? al1 : 0.0f;
                if (FX) {
                    // the fast blend forms each composite's weight once, both splats in one
                    // packed product, then rgb += col * (alpha * T) as fused multiply-adds
                    // in list order: two roundings per term like (col * alpha) * T, in
                    // another association (colours within the fast blend's 1e-5, not bit
                    // parity; no decision reads them).  A splat not taken, and the unused
                    // half-slot of an odd batch (AA.y = 0, zeroed colours), has weight
                    // 0 * T = 0, and fma(col, 0, acc) = acc for its finite colours
                    const f2 w = AA * TT;
                    crg = pk_fma_b_lo((f2){q3.z, q3.w}, w, crg);     // + col0 * (AA.x * TT.x)
                    crg = pk_fma_b_hi((f2){q4.x, q4.y}, w, crg);     // + col1 * (AA.y * TT.y)
                    cb = __builtin_fmaf(q4.w, w.y, __builtin_fmaf(q4.z, w.x, cb));
                } else {
                    // the three colour products, then rgb += (col * alpha) * T as fused
                    // multiply-adds in list order (render.cu:337, the contraction
                    // gsr_blend_md2 documents)
                    const f2 p0 = (f2){q3.z, q3.w} * AA.x;
                    const f2 p1 = pk_mul_b_hi((f2){q4.x, q4.y}, AA);     // col1 * AA.y
                    const f2 pb = (f2){q4.z, q4.w} * AA;
                    crg = pk_fma_b_lo(p0, TT, crg);                      // + (col0 * AA.x) * TT.x
                    crg = pk_fma_b_hi(p1, TT, crg);                      // + (col1 * AA.y) * TT.y
                    cb = __builtin_fmaf(pb.y, TT.y, __builtin_fmaf(pb.x, TT.x, cb));
                }
                if (DIAG) {
                    // splat-iterations with no taken lane; pair-iterations in which no live
                    // in-box lane of either splat passes the alpha test's exp argument
                    const float xs0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(xs_l), s0));
                    const float xs1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(xs_l), s1));
                    const bool cand0 = in0 && !(mdh.x < xs0);
                    const bool cand1 = has1 && in1 && !(TT.x < 1e-3f) && !(mdh.y < xs1);
                    dg.zero_taken += (__ballot(take0) == 0ull ? 1 : 0) + (has1 && __ballot(take1) == 0ull ? 1 : 0);
                    dg.no_cand_pairs += (__ballot(cand0 || cand1) == 0ull) ? 1 : 0;
                    dg.iter += has1 ? 2 : 1;
                    dg.active += (uint64_t)__popcll(__ballot(in0)) +
                                (uint64_t)__popcll(__ballot(in1 & !(TT.y < 1e-3f)));
                    dg.taken += (uint64_t)__popcll(__ballot(take0)) + (uint64_t)__popcll(__ballot(take1));
                    const uint32_t g0 = (uint32_t)__builtin_amdgcn_readlane((int)gi_l, s0);
                    const uint32_t g1 = (uint32_t)__builtin_amdgcn_readlane((int)gi_l, s1);
                    tcount += (take0 ? 1u : 0u) + (take1 ? 1u : 0u);
                    thash += (take0 ? take_mix(g0) : 0u) + (take1 ? take_mix(g1) : 0u);
                }
                TT.x = FX ? __builtin_fmaf(-TT.y, AA.y, TT.y) : TT.y * (1.0f - AA.y);
                // render.cu:328 for the next pair; after the batch's last pair the threshold
                // is ~3.4e35 (1e-3's bits | kLastPair), so the ballot is 0 and the loop ends:
                // the batch-end test costs two scalar instructions, not a compare of j
                const float thr = __uint_as_float(0x3a83126fu | (d1 & kLastPair));
                const uint64_t live_new = __ballot(!(TT.x < thr));
                if (FX) {
                    // n += take0 + take1 as two v_addc (the take masks as carry-in);
                    // alpha >= +0 here, so its float maximum is the u32 maximum
                    ntk = count_lanes2(ntk, t0m, t1m);
                    amax = __uint_as_float(max(max(__float_as_uint(amax), __float_as_uint(AA.x)),
                                               __float_as_uint(AA.y)));
                    // (the band checks of each pixel's T decisions run once, at the block's
                    // end, on the latched T before its last composite: no per-iteration branch)
                }
                ++j;
                live = live_new;
                if (live == 0ull) break;
            }
            }
            alive = __ballot(!(TT.x < 1e-3f)) != 0ull;   // block not yet saturated
            T = TT.x;
        } else {
            // exact one-splat path (render.cu:329-340 with gsr_blend_expf and selects)
            for (uint32_t k = 0; mm && alive; ++k) {
                const int s = __builtin_ctzll(mm);
                mm &= mm - 1;
                const uint64_t box = box_mask((uint32_t)__builtin_amdgcn_readlane((int)dsc, s));
                const float* S = wP + (k >> 1) * kSlot;
                const int h = (int)(k & 1u);
                SplatStep st;
                const bool take = splat_step(st, fpx, fpy, S[0 + h], S[2 + h], S[4 + h], S[6 + h], S[8 + h],
                                             S[10 + h], S[12 + h], box, T);
                const float alpha = st.alpha;
                const float wr = __builtin_fmaf(S[14 + 2 * h] * alpha, T, crg.x);
                const float wg = __builtin_fmaf(S[15 + 2 * h] * alpha, T, crg.y);
                const float wb = __builtin_fmaf(S[18 + h] * alpha, T, cb);
                const float Tn = T * (1.0f - alpha);
                if (DIAG) {
                    dg.iter += 1;
                    dg.slow += 1;
                    const bool in = __builtin_amdgcn_inverse_ballot_w64(box);
                    dg.active += (uint64_t)__popcll(__ballot(in & !(T < 1e-3f)));
                    dg.taken += (uint64_t)__popcll(__ballot(take));
                    tcount += take ? 1u : 0u;
                    thash += take ? take_mix((uint32_t)__builtin_amdgcn_readlane((int)gi_l, s)) : 0u;
                }
                crg.x = take ? wr : crg.x;
                crg.y = take ? wg : crg.y;
                cb = take ? wb : cb;
                T = take ? Tn : T;
                alive = __ballot(!(T < 1e-3f)) != 0ull;
            }
        }
    }
    if (FX) {
        // The band checks, once per pixel.  A pixel's n, m and tprev stop changing once
        // its T drops below 1e-3 (nothing is composited after), so at the end:
        //  - saturated: its decisive step took T from tprev (>= 1e-3) to T (< 1e-3); the
        //    exact chain takes the same branches if both lie outside the band (every
        //    earlier T is >= tprev: T never increases);
        //  - unsaturated: T must lie above the band.
        // Pixels that started saturated (outside the cover or `only`) composited nothing.
        const float B = fx_band(band0, ntk, amax);
        const float hi = 1e-3f * (1.0f + B), lo = 1e-3f * (1.0f - B);
        const bool nr = (T < 1e-3f) ? (ntk != 0u) & ((tprev < hi) | !(T < lo)) : (T < hi);
        suspect |= __ballot(nr);
    }
    if (SPLIT == 1) {
        const bool unsat = __ballot(!(T < 1e-3f)) != 0ull;
        if (unsat) tsave[lane] = T;
        if (lane == 0) {
            *flag = unsat ? 1u : 0u;
            if (unsat) atomicAdd(gate, 1u);
        }
        suspect = unsat ? 1ull : 0ull;   // returned: the caller flags a speculative frame
    }
    // FX: every pixel but the suspect ones; exact: the pixels of `only`
    const bool write = FX ? ((suspect >> lane) & 1ull) == 0ull : mine;
    if (write && px < W && py < H) {
        const size_t o = (size_t)py * (size_t)W + (size_t)px;
        const size_t hw = (size_t)W * (size_t)H;
        out[o] = inside ? crg.x : 0.0f;
        out[hw + o] = inside ? crg.y : 0.0f;
        out[2 * hw + o] = inside ? cb : 0.0f;
        if (DIAG && tmap) tmap[o] = (uint64_t)tcount | ((uint64_t)thash << 32);
    }
    return suspect;
}

// One-wave workgroups: workgroup g blends one 8x8 block, so a finished block
// frees its wave slot at once (no waiting for the tile's other three waves).
// Hardware dispatch sends workgroup g to XCD g mod 8.  bands > 1: the blocks
// (tile-major, a tile's four blocks consecutive) are cut into bands of B
// consecutive blocks and band j goes to XCD j mod 8, so each XCD's L2 serves runs
// of neighbouring tiles while heavy and light image regions spread over all XCDs;
// padding workgroups past the last block exit.  bands <= 1: one contiguous run of
// blocks per XCD (xcd_chunk).
// FX: fast-exp blend; a block it cannot vouch for is blended again exactly by the
// same wave (counters[8] blocks, counters[9] suspect pixels, with diagnostics).
// STAMPS (timeline diagnostics, no counters): counters[2 * g] = start of the
// s_memrealtime clock (100 MHz), counters[2 * g + 1] = duration (40 bits) |
// placement << 40 (XCC id and HW_ID's SE / SH / CU / SIMD / slot).
// DIAG: counters[0..9], then the take map (one u64 per pixel) from counters + 16.
// SPLIT: the depth split's phase A (1) or B (2), blend_block; phase B's workgroup 0
// publishes the count of blocks phase A left unsaturated (sp.host_st), and every
// workgroup returns at once when that count is 0 or its own block is saturated.
template <bool DIAG, bool STAMPS, bool FX, int SPLIT>
__global__ __launch_bounds__(64, 8) void k_blend_w(const uint32_t* __restrict__ idx,
                                                 const uint2* __restrict__ ranges,
                                                 const uint4* __restrict__ rec, int tiles_x, int tiles_y,
                                                 int W, int H, int cover_w, int cover_h,
                                                 float* __restrict__ out,
                                                 unsigned long long* __restrict__ counters, int bands,
                                                 float band0, BlendSplit sp) {
    __shared__ float4 sP[32 * 24 / 4];
    const int ntiles = tiles_x * tiles_y;
    const int vb = (int)blockIdx.x;
    if (SPLIT == 1 && vb == 0 && threadIdx.x == 0 && sp.cut.kcut) split_cut_update(sp.cut);
    if (SPLIT == 2) {
        const uint32_t g = *sp.gate;   // uniform
        if (vb == 0 && threadIdx.x == 0 && sp.host_st) {
            // a frame whose near part fell short of the split point by more than 1/16 (its
            // threshold was extrapolated from a smaller point, split_cut_update) says
            // nothing about that point: its tag's low half 0xffff matches no split point
            // (<= 1000), so the controller waits for a frame with a measured threshold
            // rather than grow twice on one miss
            const bool short_near = sp.cut.nnear && *sp.cut.nnear < sp.cut.na - sp.cut.na / 16u;
            sp.host_st->split_unsat = g;
            sp.host_st->split_pm = short_near ? (sp.pm | 0xffffu) : sp.pm;
            __threadfence_system();
        }
        if (g == 0u) return;
    }
    int L;
    if (!blend_block_index(vb, ntiles, bands, L)) return;
    if (SPLIT == 2 && sp.bflag[L] == 0u) return;   // saturated in phase A: its pixels are final
    const int tile = L >> 2, sub = L & 3;
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int lane = (int)(threadIdx.x & 63u);
    uint64_t t_start = 0, place = 0;
    if (STAMPS && lane == 0) {
        uint32_t hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        place = ((uint64_t)(xcc & 7u) << 16) | (hw & 0xffffu);
        t_start = __builtin_amdgcn_s_memrealtime();
        counters[2 * vb] = t_start;
    }
    const uint2 rr = ranges[tile];                          // {~start, end}, zero = empty
    const uint32_t beg = rr.y ? ~rr.x : 0u;
    const int bx = tx * GSR_TILE_PX + (sub & 1) * 8, by = ty * GSR_TILE_PX + (sub >> 1) * 8;
    uint64_t* tmap = DIAG ? reinterpret_cast<uint64_t*>(counters + 16) : nullptr;
    BlendDiag dg;
    const uint64_t redo = blend_block<DIAG, FX, SPLIT>(idx, rec, beg, rr.y, bx, by, lane, W, H, cover_w, cover_h,
                                                       out, reinterpret_cast<float*>(sP), dg, tmap, band0, ~0ull,
                                                       SPLIT ? sp.tbuf + 64 * (size_t)L : nullptr,
                                                       SPLIT ? sp.bflag + L : nullptr, sp.gate);
    if (SPLIT == 1 && redo && sp.spec_host && lane == 0) {
        sp.spec_host->spec_miss = 1u;   // no phase B queued for this frame: it is incomplete
        if (sp.fstatus) atomicOr(sp.fstatus, 4u);
        __threadfence_system();
    }
    if (FX && redo) {
        if (DIAG && lane == 0) {
            atomicAdd(counters + 8, 1ull);
            atomicAdd(counters + 9, (unsigned long long)__popcll(redo));
        }
        // only the suspect pixels (all of them after an aborted fast pass): the others
        // start saturated, so the cull drops every record that misses the suspects
        // and the wave stops once they saturate
        blend_block<DIAG, false, 0>(idx, rec, beg, rr.y, bx, by, lane, W, H, cover_w, cover_h, out,
                                 reinterpret_cast<float*>(sP), dg, tmap, 0.0f, redo);
    }
    if (STAMPS && lane == 0)
        counters[2 * vb + 1] = ((__builtin_amdgcn_s_memrealtime() - t_start) & ((1ull << 40) - 1)) | (place << 40);
    if (DIAG && lane == 0) {
        if (sub == 0 && dg.loaded) atomicAdd(counters, (unsigned long long)dg.loaded);
        atomicAdd(counters + 1, (unsigned long long)dg.iter);
        atomicAdd(counters + 2, (unsigned long long)dg.active);
        atomicAdd(counters + 3, (unsigned long long)dg.taken);
        atomicAdd(counters + 4, (unsigned long long)dg.slow);
        atomicAdd(counters + 5, (unsigned long long)dg.zero_taken);
        atomicAdd(counters + 7, (unsigned long long)dg.no_cand_pairs);
        atomicAdd(counters + 6, (unsigned long long)(dg.iter * 64));
    }
}

// Exhaustive checks behind the blend's exp (gsr_exp_probe).  Over every float key k
// in [key_lo, key_hi): viol[0] counts gsr_blend_expf(x_k) > gsr_blend_expf(x_k+1)
// (monotonicity of the exact exp, which makes the alpha test a threshold on its
// argument); viol[1] counts the x in [-2e7, 5] where a half of gsr_blend_expf_x2 differs
// from gsr_blend_expf (the packed path's unclamped domain); and over the same keys the
// largest |fast_expf / gsr_blend_expf - 1| is kept as float bits, split at x >= x_big:
// errs[0] every key (x in the range), errs[1] x >= x_big.
__global__ __launch_bounds__(256) void k_exp_probe(uint32_t key_lo, uint32_t key_hi, float x_big,
                                                   unsigned long long* __restrict__ viol,
                                                   uint32_t* __restrict__ errs) {
    const uint64_t nthr = (uint64_t)gridDim.x * blockDim.x;
    uint64_t bad = 0, pk_bad = 0;
    float emax = 0.0f, ebig = 0.0f;
    for (uint64_t k = (uint64_t)key_lo + blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; k < key_hi; k += nthr) {
        const float x = gsr_key_float((uint32_t)k);
        const float e = gsr_blend_expf(x);
        const float en = gsr_blend_expf(gsr_key_float((uint32_t)k + 1u));
        bad += e > en ? 1u : 0u;
        f2 xx;
        xx.x = x;
        xx.y = -x;
        if (x >= -2e7f && x <= 5.0f) {
            const f2 pk = gsr_blend_expf_x2(xx);
            pk_bad += __float_as_uint(pk.x) != __float_as_uint(e) ? 1u : 0u;
            if (-x >= -2e7f && -x <= 5.0f)
                pk_bad += __float_as_uint(pk.y) != __float_as_uint(gsr_blend_expf(-x)) ? 1u : 0u;
        }
        const float f = fast_expf_x2(xx).x;
        const float r = (float)fabs((double)f / (double)e - 1.0);   // rounded up below
        const float ru = __uint_as_float(__float_as_uint(r) + 1u);
        emax = fmaxf(emax, ru);
        if (x >= x_big) ebig = fmaxf(ebig, ru);
    }
    if (bad) atomicAdd(viol, (unsigned long long)bad);
    if (pk_bad) atomicAdd(viol + 1, (unsigned long long)pk_bad);
    atomicMax(errs, __float_as_uint(emax));
    atomicMax(errs + 1, __float_as_uint(ebig));
}

}  // namespace

// ------------------------------------------------------------------ launchers

hipError_t launch_blend(const uint32_t* idx, const uint2* ranges, const uint4* rec, const Frame& fr,
                        float* out, unsigned long long* consumed, bool stamps, int band_tiles, int blend_exp,
                        hipStream_t s, const BlendSplit* split) {
    // blend_exp 2 (test hook): the fast blend with a band of 100 %, so every block in
    // which a pixel saturates (or ends below 2e-3) is blended again exactly
    const bool fast_exp = blend_exp != 0;
    const float band0 = blend_exp == 2 ? 1.0f : kFxBand0;
    const int nt = fr.tiles_x * fr.tiles_y;
    if (nt <= 0) return hipSuccess;
    int bands, ng;
    blend_grid(nt, band_tiles, bands, ng);
    const int phase = split ? split->phase : 0;
    if (phase < 0 || phase > 2 || (phase && (fast_exp || stamps || !split->tbuf || !split->bflag || !split->gate)))
        return hipErrorInvalidValue;
    const BlendSplit sp = split ? *split : BlendSplit{0, nullptr, nullptr, nullptr, nullptr, nullptr, {}, 0u, nullptr};
#define GSR_BLEND_S(D, ST, FX, SP)                                                                          \
    hipLaunchKernelGGL((k_blend_w<D, ST, FX, SP>), dim3(ng), dim3(64), 0, s, idx, ranges, rec, fr.tiles_x,  \
                       fr.tiles_y, fr.W, fr.H, fr.cover_w, fr.cover_h, out, consumed, bands, band0, sp)
#define GSR_BLEND(D, ST, FX) GSR_BLEND_S(D, ST, FX, 0)
    if (phase) {
        if (consumed) {
            if (phase == 1) GSR_BLEND_S(true, false, false, 1);
            else GSR_BLEND_S(true, false, false, 2);
        } else {
            if (phase == 1) GSR_BLEND_S(false, false, false, 1);
            else GSR_BLEND_S(false, false, false, 2);
        }
    } else if (stamps && consumed) {
        if (fast_exp) GSR_BLEND(false, true, true);
        else GSR_BLEND(false, true, false);
    } else if (consumed) {
        if (fast_exp) GSR_BLEND(true, false, true);
        else GSR_BLEND(true, false, false);
    } else {
        if (fast_exp) GSR_BLEND(false, false, true);
        else GSR_BLEND(false, false, false);
    }
#undef GSR_BLEND
#undef GSR_BLEND_S
    return hipGetLastError();
}

hipError_t launch_exp_probe(uint32_t key_lo, uint32_t key_hi, float x_big, unsigned long long* viol, uint32_t* errs,
                            hipStream_t s) {
    hipLaunchKernelGGL(k_exp_probe, dim3(8192), dim3(256), 0, s, key_lo, key_hi, x_big, viol, errs);
    return hipGetLastError();
}

}  // namespace gsr

// gsr_kernels.hip — gfx950 (CDNA4) kernels of the 3DGS rasterizer's geometry stages (pipeline
// overview, kernel by kernel: DESIGN.md section 9).  Sections: AoS -> SoA, preprocess, blend
// cull words (the per-record half of the blend's cull), radix sort, emission, tile binning,
// bucket depth sort (with the depth split's k_split_sat), live partition, standalone sort
// ABI helpers (and k_xs_probe), launchers.  The blend stage: gsr_blend.hip and
// gsr_blend_derived.hip.
//
// Every float expression restates render.cu / math.cu in the same operation
// order; the file is compiled with -ffp-contract=off so no FMA is formed
// implicitly, and the transcendental functions come from gsr_detmath.h, so the
// results are bit-identical to the CPU oracle (oracle/gsr_oracle.c).
// Shared wave / workgroup helpers: gsr_device.h; probes of no stage: gsr_probes.hip.  The
// part of the preprocess its backward pass (gsr_project.hip) shares — SoaWg, the loads, the
// world-space covariance, mm3 / gemm, the cull tests: gsr_preprocess_device.h.
#include "gsr_device.h"
#include "gsr_preprocess_device.h"

namespace gsr {

namespace {

// --------------------------------------------------------------- AoS -> SoA

// Accepts the reference's Gaussian[] (gaussians.hpp:16-30) as input.
__global__ __launch_bounds__(256) void k_aos_to_soa(const gsr_gaussian* __restrict__ g, int64_t n,
                                                    float* __restrict__ a, int64_t stride) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const gsr_gaussian& q = g[i];
    a[GSR_A_X * stride + i] = q.x;
    a[GSR_A_Y * stride + i] = q.y;
    a[GSR_A_Z * stride + i] = q.z;
    a[GSR_A_OPACITY * stride + i] = q.opacity;
#pragma unroll
    for (int c = 0; c < 3; c++) a[(GSR_A_SCALE0 + c) * stride + i] = q.scale[c];
#pragma unroll
    for (int c = 0; c < 4; c++) a[(GSR_A_ROT0 + c) * stride + i] = q.rot[c];
#pragma unroll
    for (int c = 0; c < 27; c++) a[(GSR_A_SH0 + c) * stride + i] = q.sh[c];
}

// ------------------------------------------------------------------ preprocess

// (mm3, gemm, SoaWg, PreLoads / preprocess_load, preprocess_cov3d and the cull tests:
// gsr_preprocess_device.h; matVecMul4D_cuda, mv4: gsr_device.h)

// Compact tile rectangle of one Gaussian for the emission: tx0 | tx1 << 16 |
// ty0 << 32 | ty1 << 48; tile count (tx1 - tx0 + 1) * (ty1 - ty0 + 1), which
// is 0 for the dead value below (tx0 = ty0 = 1, tx1 = ty1 = 0).
constexpr uint64_t kDeadRect = 0x0000000100000001ull;
__device__ __forceinline__ uint32_t rect_count(uint64_t r) {
    const int tx0 = (int)(r & 0xffffu), tx1 = (int)((r >> 16) & 0xffffu);
    const int ty0 = (int)((r >> 32) & 0xffffu), ty1 = (int)(r >> 48);
    return (uint32_t)((tx1 - tx0 + 1) * (ty1 - ty0 + 1));
}

// 4-B form of a tile rectangle for grids of at most 256 tiles per axis (the
// binning path): tx0 | tx1 << 8 | ty0 << 16 | ty1 << 24.  Lossless there (every
// coordinate is < 256; the dead value packs to 0x00010001 and unpacks to kDeadRect).
__device__ __forceinline__ uint32_t pack_rect(uint64_t r) {
    return (uint32_t)(r & 0xffu) | (uint32_t)((r >> 8) & 0xff00u) | (uint32_t)((r >> 16) & 0xff0000u) |
           (uint32_t)((r >> 24) & 0xff000000u);
}
__device__ __forceinline__ uint64_t unpack_rect(uint32_t p) {
    return (uint64_t)(p & 0xffu) | ((uint64_t)((p >> 8) & 0xffu) << 16) | ((uint64_t)((p >> 16) & 0xffu) << 32) |
           ((uint64_t)(p >> 24) << 48);
}

// The preprocess's tile rect of Gaussian i: 8 B, or packed to 4 B (pack_rect) for the
// binning path (`packed`: the buffer then holds u32 rects in index order).
__device__ __forceinline__ void put_rect(uint64_t* rect, int64_t i, uint64_t r, int packed) {
    if (packed)
        reinterpret_cast<uint32_t*>(rect)[i] = pack_rect(r);
    else
        rect[i] = r;
}

// ------------------------------------------------------------------ blend cull words
//
// The blend culls every record of its tile list against each 8x8 block (the
// ellipse-vs-block test and the fast-path proof below).  Everything in those
// tests that depends on the record alone is computed once here, in
// k_preprocess, and stored as the record's fourth 16-B word (the blend's record
// gather fetches the whole 64-B line anyway: profiles/r01_fetch_calibration.txt):
//   { xs, ih, iv, S }
// xs   gsr_alpha_take_min_x(op): the alpha test passes on a pixel iff its exp
//      argument -md2/2 >= xs (exact, gsr_detmath.h).  The block test's md2 cutoff is
//      -2 xs (+1e-6, block_cut) when the conic is robustly positive definite; the
//      blend's fast-exp mode takes its alpha decisions from xs
//      (-inf: every pixel passes, the block test never culls)
// ih   -h / e, iv = -h / a (edge minimisers of the quadratic form), h = (b + c) / 2
// S    |a| + |b| + |c| + |e| if the record passes the per-record part of the
//      fast-path proof (robustly PD, finite S and colour, coefficients 0 or
//      >= 2^-60), else +inf (then the per-block part S M^2 <= 4e7 fails, and the
//      block test's rounding margin is infinite: conservative, never culls)

// md2 cutoff of one splat: alpha = fminf(op * exp(-md2/2), 0.99) < 1e-3 holds
// for every md2 > 2 ln(1000 op) (exp and the product are within a few ulp), so
// lanes beyond the returned bound can never composite.  The bound is padded by
// 1e-5 relative + 1e-3 absolute — orders of magnitude above the rounding of
// gsr_blend_expf, the product and the hardware log2 used here — and is NaN (never
// skip) for NaN opacity, +inf for infinite opacity, -inf for op <= 0.  It only
// decides whether a wave may SKIP work; it never changes a composited value.
__device__ __forceinline__ float md2_cutoff(float op) {
    const float l = __log2f(op * 1000.0f);                   // v_log_f32
    return (l * 1.38629436111989061f) * 1.00001f + 1e-3f;     // 2 ln2 log2(1000 op)
}

// Fast-path proof for one splat on one block (exactness, not a heuristic):
// finite conic that is robustly positive definite with |a|+|b|+|c|+|e| times
// the squared largest block offset <= 4e7 keeps every in-box md2 finite and
// >= -10 (float error of the 9-op form < 10), so -md2/2 lies in gsr_blend_expf_x2's
// proven range; finite colours make "alpha = 0 when not taken" leave the
// accumulators bit-identical (c + (col*0)*T == c, T*(1-0) == T).
// Every coefficient is also 0 or of magnitude >= 2^-60: the pixel offsets are
// integers, so every intermediate of the md2 form is a multiple of 2^-83 —
// zero or a normal number — and scaling the coefficients by -0.5 scales every
// intermediate exactly: the form on (-a/2, -b/2, -c/2, -e/2) IS -0.5f * md2.
// The per-record part is the cull word's S; the per-block part, in the blend,
// is S * M * M <= 4e7.
__device__ __forceinline__ bool coef_ok(float v) { return v == 0.0f || fabsf(v) >= 0x1p-60f; }

// xs_op(): gsr_alpha_take_min_x(op), the word's only term that depends on the opacity alone
// (k_preprocess_multi computes it once per Gaussian for all its cameras), evaluated where
// the word needs it.
template <class XsOp>
__device__ __forceinline__ uint4 cull_word_xs(float a, float b, float c, float e, XsOp xs_op, float r, float g,
                                              float bl) {
    const float inf = __builtin_huge_valf();
    const float h = 0.5f * (b + c);
    const bool pd = a > 0.0f && e > 0.0f && (a * e - h * h) > 1e-4f * (a * e);
    const float S = fabsf(a) + fabsf(b) + fabsf(c) + fabsf(e);
    const bool fast = pd && isfinite(S) && isfinite(r) && isfinite(g) && isfinite(bl) && coef_ok(a) &&
                      coef_ok(b) && coef_ok(c) && coef_ok(e);
    // edge minimisers; v_rcp_f32 (~1 ulp) moves them by ~1e-7 relative, which
    // changes an edge minimum only at second order (e * delta^2), far inside the
    // block test's rounding margin
    const float ih = pd ? -h * __builtin_amdgcn_rcpf(e) : 0.0f;
    const float iv = pd ? -h * __builtin_amdgcn_rcpf(a) : 0.0f;
    // a conic that is not robustly PD never culls: xs = -inf makes block_cut +inf.  Its
    // alpha decisions come from the exact one-splat path (no fast proof), never xs.
    const float xs = pd ? xs_op() : -inf;
    return make_uint4(__float_as_uint(xs), __float_as_uint(ih), __float_as_uint(iv), __float_as_uint(fast ? S : inf));
}
__device__ __forceinline__ uint4 cull_word(float a, float b, float c, float e, float op, float r, float g,
                                           float bl) {
    return cull_word_xs(a, b, c, e, [&] { return gsr_alpha_take_min_x(op); }, r, g, bl);
}

// Tile row spans (binning path, GSR_TUNE_TILE_SPANS).  A splat's tile rect is the
// box of its AABB, and an elongated or tilted ellipse reaches alpha >= 1e-3 on only
// part of it: config 2 lists 5.39M (tile, splat) pairs of which 4.12M can composite
// at all.  For each of the first four tile rows of the rect, nibble r of the 16-bit
// code counts the columns at the row's left end (bits 0-1) and right end (bits 2-3)
// that hold no in-box pixel of the ellipse q <= C; the row pass lists only the
// columns in between (none when left + right >= the row's width).  Rows past the
// fourth (4.1M of the 4.12M reachable pairs sit in the first four) keep every
// column; a count stops at 3, keeping the middle columns (conservative; counts up
// to 15 drop no more pairs on config 2, and 2 B per Gaussian keep the row pass's
// gather of the codes by index half the footprint of 4 B).
//
// Why a dropped pair changes no pixel.  q = a dx^2 + (b + c) dx dy + e dy^2 is the
// exact md2 of the record's float conic; the blend's float md2 is within
// 4e-6 S M^2 of it (block_may_reach's bound: S = |a|+|b|+|c|+|e|, M = largest
// |offset| in the AABB), so with C = cut + 4e-6 S M^2 + 1e-3 every pixel outside
// q <= C has float md2 > cut, alpha < 1e-3, and is never taken.  The x-extent of
// q <= C over a strip of offsets [u0, u1] is [L, R]: R is the ellipse's rightmost
// offset xr = sqrt(C e / det) when the strip holds its ordinate yr = -h xr / e,
// else (-h u + sqrt(a C - det u^2)) / a at the strip end nearer yr (R(dy) is
// concave); L mirrors it.  Float error: det = a e - h^2 is within 3e-7 k of itself
// relative (k = a e / det <= 1e4 for a finite cut), which moves xr, ym and the
// square root by at most sqrt(6e-7 (k + 1)) xr; the pads below cover that and the
// approximate rcp / sqrt (~1 ulp) with room.  A numpy restatement of this function
// (tools/sim/spans_check.py) keeps 78.7 % of config 2's pairs (the exact hull: 76.5 %)
// and every pair it drops peaks at alpha <= 0.9976e-3 on its tile.
__device__ __forceinline__ uint16_t tile_row_spans(float cx, float cy, float a, float b, float c, float e,
                                                   float cut, uint4 cw, int xmin_px, int xmax_px, int ymin_px,
                                                   int ymax_px, int tx0, int tx1, int ty0, int ty1) {
    const float S = __uint_as_float(cw.w);
    // not robustly positive definite (cut = inf) or without the fast proof (S = inf): keep all
    if (!(cut < 3.0e38f) || !(S < 3.0e38f)) return 0u;
    const float h = 0.5f * (b + c);
    const float det = a * e - h * h;   // > 1e-4 a e here (cull_word's pd test)
    const float M = fmaxf(fmaxf(fabsf((float)xmin_px - cx), fabsf((float)xmax_px - cx)),
                          fmaxf(fabsf((float)ymin_px - cy), fabsf((float)ymax_px - cy)));
    const float C = cut + (4e-6f * S * M * M + 1e-3f);
    const float rdet = __builtin_amdgcn_rcpf(det), ra = __builtin_amdgcn_rcpf(a);
    const float xr = __builtin_amdgcn_sqrtf(C * e * rdet);   // rightmost offset (leftmost: -xr)
    const float ym = __builtin_amdgcn_sqrtf(C * a * rdet);   // largest |dy| of the ellipse
    const float yr = -h * xr * __builtin_amdgcn_rcpf(e);     // its ordinate (leftmost: -yr)
    const float k = a * e * rdet;
    const float rel = __builtin_amdgcn_sqrtf(6e-7f * (k + 1.0f)) + 1e-4f;
    // offsets are exact (integer pixel minus integer-valued centre); cx + L rounds by
    // < 5e-4 px below 4096, hence the 1/64 px (a 2-px pad kept 6 % more pairs)
    const float padx = 0.015625f + rel * xr, ymp = ym * (1.0f + rel) + 0.015625f;
    const float aC = a * C;
    const int w = tx1 - tx0 + 1;
    const int rows = min(ty1 - ty0 + 1, 4);
    uint32_t code = 0;
    for (int r = 0; r < rows; r++) {
        const int ty = ty0 + r;
        const int y0 = max(ty * GSR_TILE_PX, ymin_px), y1 = min(ty * GSR_TILE_PX + (GSR_TILE_PX - 1), ymax_px);
        const float dy0 = (float)y0 - cy, dy1 = (float)y1 - cy;
        int c0 = tx1 + 1, c1 = tx0 - 1;   // empty
        if (!(dy0 > ymp || dy1 < -ymp)) {
            const float u0 = fminf(fmaxf(dy0, -ym), ym), u1 = fminf(fmaxf(dy1, -ym), ym);
            float R = xr, L = -xr;
            if (!(yr >= u0 && yr <= u1)) {
                const float u = yr < u0 ? u0 : u1;
                R = (-h * u + __builtin_amdgcn_sqrtf(fmaxf(aC - det * u * u, 0.0f))) * ra;
            }
            if (!(-yr >= u0 && -yr <= u1)) {
                const float u = -yr < u0 ? u0 : u1;
                L = (-h * u - __builtin_amdgcn_sqrtf(fmaxf(aC - det * u * u, 0.0f))) * ra;
            }
            const float xl = fmaxf(cx + L - padx, (float)xmin_px), xh = fminf(cx + R + padx, (float)xmax_px);
            if (xl <= xh) {
                c0 = max(tx0, (int)floorf(xl * (1.0f / GSR_TILE_PX)));
                c1 = min(tx1, (int)floorf(xh * (1.0f / GSR_TILE_PX)));
            }
        }
        int sl, sr;
        if (c0 > c1) {
            sl = sr = min(w, 3);   // no column reachable (w > 6: the middle ones stay)
        } else {
            sl = min(c0 - tx0, 3);
            sr = min(tx1 - c1, 3);
        }
        code |= (uint32_t)(sl | (sr << 2)) << (4 * r);
    }
    return (uint16_t)code;
}

// preprocess_one in three parts, shared with k_preprocess_multi: the loads (preprocess_load,
// gsr_preprocess_device.h), the view-independent arithmetic (preprocess_cov3d there, and the
// opacity-only terms, PreShared) and everything that depends on the camera
// (preprocess_camera).
//
// What k_preprocess_multi computes once per Gaussian for all its cameras (3D scenes: the
// record's opacity is the scene's).
struct PreShared {
    float cov[9];   // preprocess_cov3d
    float xs;       // gsr_alpha_take_min_x(op)
    float cut;      // md2_cutoff(op)
};

// The camera-dependent part for Gaussian i against frame fr.  PRE: the view-independent
// values come from *pre (else they are computed where they are first needed), and the SH-3
// coefficients from sh3, loaded on the first camera that keeps the Gaussian (*have_sh3).
// kcut and far_pass by reference, and the dead item through a named pointer: with these
// k_preprocess<false, *> compile to the instructions they had as one function
// (tools/kernel_isa_diff.py).
template <bool T4D, bool SH3, bool PRE>
__device__ __forceinline__ uint32_t preprocess_camera(const SoaWg& A, const PreLoads<T4D, SH3>& L,
                                                      const PreShared* pre, float* sh3, bool* have_sh3,
                                                      const Frame& fr, uint4* rec, uint64_t* items,
                                                      uint64_t* rect, int packed, uint16_t* spans,
                                                      const RecSplit& rs, const uint32_t& kcut, const bool& far_pass, int64_t i) {
    constexpr bool kEarlySH = PreLoads<T4D, SH3>::kEarlySH;
    const float gx = L.gx, gy = L.gy, gz = L.gz, tfac = L.tfac;
    const float* q_in = L.q_in;
    const float* s_in = L.s_in;
    const float op_in = L.op_in;
    const float* sh_in = L.sh_in;
    uint4* R = rec + 4 * i;
    if (!far_pass) {
        uint64_t* const dead = items + i;
        *dead = ((uint64_t)0xffffffffu << 32) | (uint64_t)(uint32_t)i;
    }

    // ---- view + clip transform and cull (render.cu:535-556) ----
    const float old_xyz[4] = {gx, gy, gz, 1.0f};
    float tmp_xyz[4], new_xyz[4];
    mv4(fr.V, old_xyz, tmp_xyz);
    if (GSR_VIEW_CULLED(tmp_xyz)) {
        if (!far_pass) put_rect(rect, i, kDeadRect, packed);
        return 0xffffffffu;
    }
    mv4(fr.P, tmp_xyz, new_xyz);
    new_xyz[0] = new_xyz[0] / new_xyz[3];
    new_xyz[1] = new_xyz[1] / new_xyz[3];
    new_xyz[2] = new_xyz[2] / new_xyz[3];
    if (GSR_CLIP_CULLED(fr, tmp_xyz, new_xyz)) {
        if (!far_pass) put_rect(rect, i, kDeadRect, packed);
        return 0xffffffffu;
    }

    // ---- 2D covariance (render.cu:655-686) ----
    const float X = tmp_xyz[0], Y = tmp_xyz[1], Z = tmp_xyz[2];
    const float fx = fr.fx, fy = fr.fy;
    float jac[6], jacT[6];
    jac[0] = fx / Z; jac[1] = 0.0f;
    jac[2] = -fx * X / (Z * Z); jac[3] = 0.0f;
    jac[4] = fy / Z; jac[5] = -fy * Y / (Z * Z);
    jacT[0] = jac[0]; jacT[1] = jac[3]; jacT[2] = jac[1];
    jacT[3] = jac[4]; jacT[4] = jac[2]; jacT[5] = jac[5];

    float tmp[9], cov[9];
    if (PRE) {
#pragma unroll
        for (int k = 0; k < 9; k++) cov[k] = pre->cov[k];
    } else {
        preprocess_cov3d(q_in, s_in, cov);
    }
    mm3(fr.Rc, cov, tmp);
    mm3(tmp, fr.RcT, cov);
    gemm<2, 3, 3>(jac, cov, tmp);
    float S2[4];
    gemm<2, 2, 3>(tmp, jacT, S2);
    const int W = fr.W, H = fr.H;
    S2[0] = (W * 0.5f) * (W * 0.5f) * S2[0];
    S2[1] = (W * 0.5f) * (H * 0.5f) * S2[1];
    S2[2] = (H * 0.5f) * (W * 0.5f) * S2[2];
    S2[3] = (H * 0.5f) * (H * 0.5f) * S2[3];
    const float det = S2[0] * S2[3] - S2[1] * S2[2];
    if (GSR_DET_CULLED(det)) {                                  // render.cu:690
        if (!far_pass) put_rect(rect, i, kDeadRect, packed);
        return 0xffffffffu;
    }
    const float invDet = 1.0f / det;
    const float ic0 = S2[3] * invDet, ic1 = -S2[1] * invDet;
    const float ic2 = -S2[2] * invDet, ic3 = S2[0] * invDet;
    if (T4D) {
        // temporal cull (exact): opacity below 0.9e-3 with a robustly positive
        // definite conic keeps md2 >= -0.05 at every pixel of the AABB, so alpha
        // = min(op exp(-md2/2), 0.99) < 1e-3 everywhere and the splat never composites
        const float opt = op_in * tfac;
        const float hh = 0.5f * (ic1 + ic2);
        if (opt < 0.9e-3f && ic0 > 0.0f && ic3 > 0.0f && (ic0 * ic3 - hh * hh) > 1e-4f * (ic0 * ic3)) {
            if (!far_pass) put_rect(rect, i, kDeadRect, packed);
            return 0xffffffffu;
        }
    }

    // ---- extent (render.cu:704-764) ----
    const float sxy = 0.5f * (S2[1] + S2[2]);
    const float tr = S2[0] + S2[3];
    const float dif = S2[0] - S2[3];
    const float rad = sqrtf(fmaxf(0.0f, dif * dif + 4 * sxy * sxy));
    float l1 = 0.5f * (tr + rad);
    float l2 = 0.5f * (tr - rad);
    l1 = fmaxf(l1, 1e-8f);
    l2 = fmaxf(l2, 1e-8f);
    const float theta = 0.5f * gsr_atan2f(2 * sxy, dif);
    const float r1 = fr.k * sqrtf(l1);
    const float r2 = fr.k * sqrtf(l2);
    const float c = gsr_cosf(theta);
    const float sn = gsr_sinf(theta);
    float ex = fabsf(r1 * c) + fabsf(r2 * sn);
    float ey = fabsf(r1 * sn) + fabsf(r2 * c);
    ex /= W / 2.0f;
    ey /= H / 2.0f;
    float xmin = new_xyz[0] - ex, xmax = new_xyz[0] + ex;
    float ymin = new_xyz[1] - ey, ymax = new_xyz[1] + ey;
    if (xmax < -0.99f || xmin > 0.99f || ymax < -0.99f || ymin > 0.99f) {   // render.cu:737
        if (!far_pass) put_rect(rect, i, kDeadRect, packed);
        return 0xffffffffu;
    }
    xmin = fmaxf(xmin, -1.0f);
    xmax = fminf(xmax, 1.0f);
    ymin = fmaxf(ymin, -1.0f);
    ymax = fminf(ymax, 1.0f);
    const int xmin_px = gsr_f2i_sat(floorf(((xmin + 1.0f) * 0.5f) * W));
    const int xmax_px = gsr_f2i_sat(ceilf(((xmax + 1.0f) * 0.5f) * W));
    const int ymin_px = gsr_f2i_sat(floorf(((ymin + 1.0f) * 0.5f) * H));
    const int ymax_px = gsr_f2i_sat(ceilf(((ymax + 1.0f) * 0.5f) * H));
    const int px_x = gsr_f2i_sat(roundf(((new_xyz[0] + 1.0f) * 0.5f) * W));
    const int px_y = gsr_f2i_sat(roundf(((new_xyz[1] + 1.0f) * 0.5f) * H));
    const uint32_t key = gsr_f2u_sat(-Z * 1e6f);                // render.cu:850

    // internal GSR_TILE_PX tiles covered (output is tile-invariant)
    const int tx0 = xmin_px / GSR_TILE_PX;
    const int tx1 = min(fr.tiles_x - 1, xmax_px / GSR_TILE_PX);
    const int ty0 = ymin_px / GSR_TILE_PX;
    const int ty1 = min(fr.tiles_y - 1, ymax_px / GSR_TILE_PX);
    const uint64_t trect =
        (uint64_t)((uint32_t)tx0 | ((uint32_t)tx1 << 16)) | ((uint64_t)((uint32_t)ty0 | ((uint32_t)ty1 << 16)) << 32);
    if (rs.mode == 1 && key >= kcut && !spans) {
        // far (key mode): no record unless phase B needs it (mode 2 writes it then)
        put_rect(rect, i, trect, packed);
        items[i] = ((uint64_t)key << 32) | (uint64_t)(uint32_t)i;
        return key;
    }
    if (far_pass && key < kcut) return key;

    // ---- SH colour, bands 0..2 (render.cu:500-534), only for survivors ----
    float dir[3] = {gx - fr.campos[0], gy - fr.campos[1], gz - fr.campos[2]};
    {
        const float nn = sqrtf(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2]);  // math.cu:7-18
        if (nn > 1e-8f) {
            dir[0] /= nn; dir[1] /= nn; dir[2] /= nn;
        } else {
            dir[0] = 0.0f; dir[1] = 0.0f; dir[2] = 0.0f;
        }
    }
    const float x = dir[0], y = dir[1], z = dir[2];
    const float xx = x * x, yy = y * y, zz = z * z;
    const float xy = x * y, yz = y * z, xz = x * z;
    const float C2_0 = 1.0925484305920792f, C2_1 = -1.0925484305920792f, C2_2 = 0.31539156525252005f,
                C2_3 = -1.0925484305920792f, C2_4 = 0.5462742152960396f;
    float col[3];
    if (PRE && SH3 && !*have_sh3) {
#pragma unroll
        for (int k = 0; k < 48; k++) sh3[k] = A(GSR_A_SH0 + k);
        *have_sh3 = true;
    }
    if (!SH3) {
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            auto SH = [&](int k) { return kEarlySH ? sh_in[ch + k] : A(GSR_A_SH0 + ch + k); };   // sh[ch], sh[3+ch], ...
            float cc = SH(0) * kShC0;
            cc += kShC1 * z * SH(6);
            cc -= kShC1 * y * SH(3);
            cc -= kShC1 * x * SH(9);
            cc += C2_0 * xy * SH(12);
            cc += C2_1 * yz * SH(15);
            cc += C2_2 * (2.0f * zz - xx - yy) * SH(18);
            cc += C2_3 * xz * SH(21);
            cc += C2_4 * (xx - yy) * SH(24);
            cc += 0.5f;
            col[ch] = fminf(fmaxf(cc, 0.0f), 1.0f);
        }
    } else {
        // "Inria-correct" mode: degree-3 SH as the 3DGS training code evaluates it
        // (left-to-right, bands 0..3), + 0.5, clamped at 0 only
        const float C3_0 = -0.5900435899266435f, C3_1 = 2.890611442640554f, C3_2 = -0.4570457994644658f,
                    C3_3 = 0.3731763325901154f, C3_4 = -0.4570457994644658f, C3_5 = 1.445305721320277f,
                    C3_6 = -0.5900435899266435f;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            auto S = [&](int k) { return PRE ? sh3[ch + 3 * k] : A(GSR_A_SH0 + ch + 3 * k); };   // coefficient k of channel ch
            float r = kShC0 * S(0);
            r = r - kShC1 * y * S(1) + kShC1 * z * S(2) - kShC1 * x * S(3);
            r = r + C2_0 * xy * S(4) + C2_1 * yz * S(5) + C2_2 * (2.0f * zz - xx - yy) * S(6) +
                C2_3 * xz * S(7) + C2_4 * (xx - yy) * S(8);
            r = r + C3_0 * y * (3.0f * xx - yy) * S(9) + C3_1 * xy * z * S(10) +
                C3_2 * y * (4.0f * zz - xx - yy) * S(11) + C3_3 * z * (2.0f * zz - 3.0f * xx - 3.0f * yy) * S(12) +
                C3_4 * x * (4.0f * zz - xx - yy) * S(13) + C3_5 * z * (xx - yy) * S(14) +
                C3_6 * x * (xx - 3.0f * yy) * S(15);
            r += 0.5f;
            col[ch] = fmaxf(r, 0.0f);
        }
    }
    const float opacity = T4D ? op_in * tfac : op_in;

    R[0] = make_uint4(__float_as_uint(ic0), __float_as_uint(ic1), __float_as_uint(ic2), __float_as_uint(ic3));
    R[1] = make_uint4(__float_as_uint(opacity), __float_as_uint(col[0]), __float_as_uint(col[1]),
                      __float_as_uint(col[2]));
    // centre pixel stored as the float the blend computes with ((float)px, render.cu:329)
    R[2] = make_uint4(__float_as_uint((float)px_x), __float_as_uint((float)px_y), (uint32_t)xmin_px | ((uint32_t)xmax_px << 16),
                      (uint32_t)ymin_px | ((uint32_t)ymax_px << 16));
    const uint4 cw = PRE ? cull_word_xs(ic0, ic1, ic2, ic3, [&] { return pre->xs; }, col[0], col[1], col[2])
                         : cull_word(ic0, ic1, ic2, ic3, opacity, col[0], col[1], col[2]);
    R[3] = cw;
    if (far_pass) return key;
    if (spans)
        spans[i] = tile_row_spans((float)px_x, (float)px_y, ic0, ic1, ic2, ic3,
                                  cw.x == __float_as_uint(-__builtin_huge_valf()) ? __builtin_huge_valf()
                                  : PRE                                           ? pre->cut
                                                                                  : md2_cutoff(opacity),
                                  cw, xmin_px, xmax_px, ymin_px, ymax_px, tx0, tx1, ty0, ty1);
    put_rect(rect, i, trect, packed);
    items[i] = ((uint64_t)key << 32) | (uint64_t)(uint32_t)i;
    return key;
}

// One Gaussian i < n; returns the depth key of its item (0xFFFFFFFF: culled or dead).
template <bool T4D, bool SH3>
__device__ __forceinline__ uint32_t preprocess_one(const SoaWg& A,
                                                   const Frame& fr, uint4* __restrict__ rec,
                                                   uint64_t* __restrict__ items, uint64_t* __restrict__ rect,
                                                   int packed, uint16_t* __restrict__ spans, float tnow,
                                                   const RecSplit& rs, int64_t i) {
    // depth split, key mode (RecSplit): 1 = records of the near Gaussians only, 2 = the
    // far ones' records only (no item, rect or span writes: those are sorted already)
    const bool far_pass = rs.mode == 2;
    if (far_pass && rs.gate && *rs.gate == 0u) return 0xffffffffu;
    const uint32_t kcut = rs.mode == 1 ? *rs.kcut : far_pass ? *rs.kcut_frame : 0xffffffffu;
    // the frame's threshold, for the far record pass (the near sort copies it too)
    if (rs.mode == 1 && i == 0) *rs.kcut_frame = kcut;
    PreLoads<T4D, SH3> L;
    preprocess_load<T4D, SH3>(A, tnow, L);
    return preprocess_camera<T4D, SH3, false>(A, L, nullptr, nullptr, nullptr, fr, rec, items, rect, packed, spans,
                                              rs, kcut, far_pass, i);
}

template <bool T4D, bool SH3>
__global__ __launch_bounds__(256) void k_preprocess(const float* __restrict__ arr, int64_t stride,
                                                    int64_t n, Frame fr, uint4* __restrict__ rec,
                                                    uint64_t* __restrict__ items, uint64_t* __restrict__ rect,
                                                    int packed, uint16_t* __restrict__ spans,
                                                    float tnow, RecSplit rs) {
    GSR_GEOM_PRIO();
    const int64_t i0 = (int64_t)blockIdx.x * 256;
    const int64_t i = i0 + threadIdx.x;
    if (i >= n) return;
    const SoaWg A{arr + i0, stride, 4u * threadIdx.x};
    (void)preprocess_one<T4D, SH3>(A, fr, rec, items, rect, packed, spans, tnow, rs, i);
}

// One Gaussian against the NC cameras of a camera path's frames in flight (3D scene blocks,
// no depth split): the scene is read once and the view-independent part computed once, and
// each camera's part runs as in k_preprocess into that camera's own outputs.
struct PreOut {
    uint4* rec;
    uint64_t* items;
    uint64_t* rect;
    uint16_t* spans;   // nullable; used with packed rects only (as launch_preprocess)
    int packed;
};
template <int NC>
struct PreMulti {
    Frame fr[NC];
    PreOut out[NC];
};

template <bool SH3, int NC>
__global__ __launch_bounds__(256) void k_preprocess_multi(const float* __restrict__ arr, int64_t stride, int64_t n,
                                                          const PreMulti<NC> m) {
    GSR_GEOM_PRIO();
    const int64_t i0 = (int64_t)blockIdx.x * 256;
    const int64_t i = i0 + threadIdx.x;
    if (i >= n) return;
    const SoaWg A{arr + i0, stride, 4u * threadIdx.x};
    PreLoads<false, SH3> L;
    preprocess_load<false, SH3>(A, 0.0f, L);
    PreShared pre;
    preprocess_cov3d(L.q_in, L.s_in, pre.cov);
    pre.xs = gsr_alpha_take_min_x(L.op_in);
    pre.cut = md2_cutoff(L.op_in);
    float sh3[SH3 ? 48 : 1];
    bool have_sh3 = false;
    const RecSplit rs{0, nullptr, nullptr, nullptr};
    const uint32_t kcut = 0xffffffffu;
    const bool far_pass = false;
#pragma unroll
    for (int c = 0; c < NC; c++)
        (void)preprocess_camera<false, SH3, true>(A, L, &pre, sh3, &have_sh3, m.fr[c], m.out[c].rec, m.out[c].items,
                                                  m.out[c].rect, m.out[c].packed, m.out[c].spans, rs, kcut, far_pass,
                                                  i);
}

// ------------------------------------------------------------------ radix sort
//
// Stable LSD pass, reduce-then-scan (no inter-workgroup spin waits, so no
// forward-progress assumption): upsweep histograms per workgroup chunk,
// per-digit scan over workgroups, downsweep that ranks each 4096-item tile with
// wave64 ballot matching (the AMD stand-in for __match_any), scatters into LDS
// in digit order and writes runs out coalesced.

// (the depth-sort pass plan — dstats, depth_pass_skipped, depth_passes_run, depth_sorted —
// is in gsr_device.h: the blend's depth split reads the sorted order too)

// SortRange (depth split, key mode; all fields null / 0 otherwise):
//   base   the far part's positions [*base, n_host) are sorted on their own (n_dev unused)
//   gate   every kernel of the pass returns at once when *gate is 0 (phase B not needed)
//   filter pass 0 reads all n_host items of the preprocess order and keeps only those with
//          key < *kcut (1, the near part) or key >= *kcut (2, the far part), written from
//          position 0 (near) or *base (far); the near pass's downsweep stores the kept
//          count in *count_out, and its upsweep copies *kcut to *kcut_copy (the frame's
//          threshold, for phase B)
//   sat    (far pass 0) also drop an item whose tile rect (rect[position], packed) holds
//          no tile phase A left unsaturated: sat is the summed-area table of those tiles,
//          (tiles_y + 1) x sat_w words, sat_w = tiles_x + 1 (k_split_sat)
//   count  with base: the far part's length (the far pass 0's kept count), else n_host - base
struct SortRange {
    const uint32_t* base;
    const uint32_t* gate;
    const uint32_t* kcut;
    int filter;
    uint32_t* count_out;
    uint32_t* kcut_copy;
    const uint32_t* sat;
    int sat_w;
    const uint32_t* rect;
    const uint32_t* count;
};

// Some tile of the packed rect pr (tx0 | tx1 << 8 | ty0 << 16 | ty1 << 24) is counted
// in the summed-area table (dead rects hold none).
__device__ __forceinline__ bool rect_hits(const uint32_t* __restrict__ sat, int w, uint32_t pr) {
    const uint32_t x0 = pr & 0xffu, x1 = (pr >> 8) & 0xffu, y0 = (pr >> 16) & 0xffu, y1 = pr >> 24;
    if (x0 > x1 || y0 > y1) return false;
    const uint32_t* r0 = sat + (size_t)y0 * (uint32_t)w;
    const uint32_t* r1 = sat + (size_t)(y1 + 1u) * (uint32_t)w;
    return r1[x1 + 1u] - r0[x1 + 1u] - r1[x0] + r0[x0] != 0u;
}

__device__ __forceinline__ bool sort_keep(const SortRange& sr, uint32_t K, uint64_t v, uint32_t pr) {
    const uint32_t k = (uint32_t)(v >> 32);
    if (sr.filter == 1) return k < K;
    return sr.filter == 0 || (k >= K && (!sr.sat || rect_hits(sr.sat, sr.sat_w, pr)));
}

__device__ __forceinline__ uint64_t sort_len(const SortRange& sr, const uint32_t* n_dev, uint32_t n_host) {
    if (sr.base) {
        const uint32_t base = min(*sr.base, n_host);
        return sr.count ? (uint64_t)min(*sr.count, n_host - base) : (uint64_t)(n_host - base);
    }
    return n_dev ? (uint64_t)*n_dev : (uint64_t)n_host;
}

template <int ITEMS, bool FILT>   // FILT: a filtered pass 0 (SortRange::filter != 0)
__global__ __launch_bounds__(kSortThreads) void k_radix_upsweep(const uint64_t* __restrict__ in,
                                                                const uint32_t* __restrict__ n_dev,
                                                                uint32_t n_host, int shift, uint32_t mask,
                                                                int groups, uint32_t* __restrict__ hist,
                                                                uint32_t* __restrict__ dstats, int pass,
                                                                SortRange sr) {
    GSR_GEOM_PRIO();
    __shared__ uint32_t h[4][FILT ? 257 : 256];   // [256]: items a filtered pass 0 drops
    __shared__ uint32_t s_st[4];
    if (sr.gate && *sr.gate == 0u) return;
    if (depth_pass_skipped(dstats, pass)) return;
    const uint32_t t = threadIdx.x;
    const uint32_t w = t >> 6;
    const bool plan = dstats && pass == 0;
    uint32_t inv_min = 0, kmax = 0, lowones = 0, any = 0;
    if (plan && t < 4) s_st[t] = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) h[k][t] = 0;
    __syncthreads();
    const uint32_t K = FILT ? *sr.kcut : 0u;
    if (FILT && sr.filter == 1 && sr.kcut_copy && blockIdx.x == 0 && t == 0) *sr.kcut_copy = K;
    const uint32_t base = sr.base ? *sr.base : 0u;
    if (!FILT) in += base;
    const uint64_t n = FILT ? (uint64_t)n_host : sort_len(sr, n_dev, n_host);
    // (XCD-contiguous chunks, so that a histogram row's 64-B lines merge in one L2, measured
    // slower: config 3 upsweep 11.5 -> 16.5 us, profiles/r05_kt_xcd_hist.txt)
    const int chunk = (int)blockIdx.x;
    uint64_t b, e;
    chunk_range(n, groups, chunk, kSortThreads * ITEMS, b, e);
    const bool masked = FILT && sr.sat;   // the far pass 0's rect test reads rect[position]
    // the digit's counter, or the drop counter for an item a filtered pass 0 does not keep
    auto dig = [&](uint64_t v, uint64_t i) {
        return !FILT || sort_keep(sr, K, v, masked ? sr.rect[i] : 0u) ? ((uint32_t)(v >> shift) & mask) : 256u;
    };
    auto note = [&](uint64_t v, uint64_t i) {
        const uint32_t k = (uint32_t)(v >> 32);
        if (k != 0xffffffffu && (!FILT || sort_keep(sr, K, v, masked ? sr.rect[i] : 0u))) {
            inv_min = max(inv_min, ~k);
            kmax = max(kmax, k);
            any = 1u;
            lowones |= ((k & 0xffu) == 0xffu ? 2u : 0u) | ((k & 0xffffu) == 0xffffu ? 4u : 0u) |
                       ((k & 0xffffffu) == 0xffffffu ? 8u : 0u);
        }
    };
    uint64_t i = b + t;
    for (; i + 3 * kSortThreads < e; i += 4 * kSortThreads) {
        const uint64_t v0 = in[i], v1 = in[i + kSortThreads], v2 = in[i + 2 * kSortThreads],
                       v3 = in[i + 3 * kSortThreads];
        atomicAdd(&h[w][dig(v0, i)], 1u);
        atomicAdd(&h[w][dig(v1, i + kSortThreads)], 1u);
        atomicAdd(&h[w][dig(v2, i + 2 * kSortThreads)], 1u);
        atomicAdd(&h[w][dig(v3, i + 3 * kSortThreads)], 1u);
        if (plan) {
            note(v0, i);
            note(v1, i + kSortThreads);
            note(v2, i + 2 * kSortThreads);
            note(v3, i + 3 * kSortThreads);
        }
    }
    for (; i < e; i += kSortThreads) {
        const uint64_t v = in[i];
        atomicAdd(&h[w][dig(v, i)], 1u);
        if (plan) note(v, i);
    }
    if (plan) {   // wave reductions first: one LDS atomic per wave and word
        inv_min = wave_max_u32(inv_min);
        kmax = wave_max_u32(kmax);
        lowones = wave_or_u32(lowones);
        any = wave_or_u32(any);
        if ((t & 63u) == 0) {
            atomicMax(&s_st[0], inv_min);
            atomicMax(&s_st[1], kmax);
            atomicOr(&s_st[2], lowones);
            atomicOr(&s_st[3], any);
        }
    }
    __syncthreads();
    hist[t * (uint32_t)groups + chunk] = h[0][t] + h[1][t] + h[2][t] + h[3][t];
    // per-workgroup plan words after the 4 final ones; pass 0's scan kernel
    // reduces them (plain stores: ~500 device atomics on 4 addresses serialise)
    if (plan && t < 4) dstats[4 + 4 * blockIdx.x + t] = s_st[t];
}

// One workgroup per digit: exclusive scan of hist[d][0..groups) in place.
__global__ __launch_bounds__(256) void k_radix_scan(uint32_t* __restrict__ hist, int groups,
                                                     uint32_t* __restrict__ totals,
                                                     const uint32_t* __restrict__ dstats, int pass,
                                                     const uint32_t* __restrict__ gate) {
    GSR_GEOM_PRIO();
    __shared__ uint32_t scratch[4];
    if (gate && *gate == 0u) return;
    if (dstats && pass == 0 && blockIdx.x == 0) {
        // reduce the upsweep's per-workgroup plan words into dstats[0..3]
        __shared__ uint32_t r[4];
        if (threadIdx.x < 4) r[threadIdx.x] = 0;
        __syncthreads();
        uint32_t a = 0, b = 0, c = 0, d = 0;
        for (int g = threadIdx.x; g < groups; g += 256) {
            const uint32_t* q = dstats + 4 + 4 * g;
            a = max(a, q[0]);
            b = max(b, q[1]);
            c |= q[2];
            d |= q[3];
        }
        a = wave_max_u32(a);
        b = wave_max_u32(b);
        c = wave_or_u32(c);
        d = wave_or_u32(d);
        if ((threadIdx.x & 63u) == 0) {
            atomicMax(&r[0], a);
            atomicMax(&r[1], b);
            atomicOr(&r[2], c);
            atomicOr(&r[3], d);
        }
        __syncthreads();
        if (threadIdx.x < 4) const_cast<uint32_t*>(dstats)[threadIdx.x] = r[threadIdx.x];
    }
    if (depth_pass_skipped(dstats, pass)) return;
    uint32_t* row = hist + (size_t)blockIdx.x * groups;
    const int per = (groups + 255) / 256;
    const int b = threadIdx.x * per;
    // every load of the thread's segment in flight at once (a loop over `per` waited for
    // each in turn: 5 round trips at 5M items, 20 for the row scan below)
    constexpr int kPerMax = kMaxSortGroups / 256;
    uint32_t v[kPerMax], local = 0;
#pragma unroll
    for (int k = 0; k < kPerMax; k++) {
        v[k] = k < per && b + k < groups ? row[b + k] : 0u;
        local += v[k];
    }
    uint32_t total;
    uint32_t run = block_exclusive_scan<uint32_t>(local, scratch, total);
#pragma unroll
    for (int k = 0; k < kPerMax; k++)
        if (k < per && b + k < groups) {
            row[b + k] = run;
            run += v[k];
        }
    if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

// pay_out != nullptr (depth sort feeding the tile binning): every pass carries
// each item's tile rectangle as a 4-B payload (pack_rect: grids <= 256 tiles per
// axis) and writes it at the item's destination, so the pass that turns out to be
// the last one leaves the rects in depth order (pay_out[np & 1] for np passes run)
// for the row pass to read coalesced.  Pass 0 takes it from the live partition's
// payloads (pay_in), or from the preprocess's packed rects: rect[position] when its
// input is the preprocess order (rect_direct: item j has index j), else rect[index]
// (a repeated sort).
// Payloads leave through the items' LDS slots, in the same digit runs.
// (The rects used to be gathered in the last pass only: a random 8-B read per item
// that cost the 5M-Gaussian frame 76 us of its 110-us pass, profiles/r02_geom_pmc.txt.)
template <int ITEMS, bool RA, bool FILT>   // FILT: a filtered pass 0 (SortRange::filter != 0)
__global__ __launch_bounds__(kSortThreads) void k_radix_downsweep(
    const uint64_t* __restrict__ in, uint64_t* __restrict__ out, const uint32_t* __restrict__ n_dev,
    uint32_t n_host, int shift, int bits, int groups, const uint32_t* __restrict__ hist,
    const uint32_t* __restrict__ totals, uint2* __restrict__ ranges, const uint32_t* __restrict__ dstats,
    int pass, const uint32_t* __restrict__ rect, int rect_direct, const uint32_t* __restrict__ pay_in,
    uint32_t* __restrict__ pay_out, SortRange sr) {
    GSR_GEOM_PRIO();
    constexpr int kTile = kSortThreads * ITEMS;
    __shared__ uint64_t s_items[kTile];
    if (sr.gate && *sr.gate == 0u) return;
    if (depth_pass_skipped(dstats, pass)) return;
    if (sr.base) {   // far part: the outputs start at *base, and so do the inputs unless filtered
        const uint32_t base = *sr.base;
        out += base;
        if (pay_out) pay_out += base;
        if (!FILT) {
            in += base;
            if (pay_in) pay_in += base;
        }
    }
    const uint32_t K = FILT ? *sr.kcut : 0u;
    const bool carry = pay_out != nullptr;
    __shared__ uint32_t s_wc[4][256];           // per-wave digit counters, then wave slot bases
    __shared__ uint32_t s_gd[256];              // per digit: global offset minus tile slot
    __shared__ uint32_t s_scr[4];
    // up to 8 items per thread the payloads get slots of their own (+8 KB of LDS, no
    // occupancy change) and travel with the items; at 16 the LDS is the occupancy
    // limit, so they reuse the items' slots in a second round (two more barriers)
    constexpr bool kPaySlots = ITEMS <= 8;
    __shared__ uint32_t s_payd[kPaySlots ? kTile : 1];
    const uint32_t t = threadIdx.x;
    const uint32_t lane = lane_id();
    const uint32_t w = t >> 6;
    const uint32_t mask = (1u << bits) - 1u;
    const uint64_t n = FILT ? (uint64_t)n_host : sort_len(sr, n_dev, n_host);
    uint64_t b, e;
    const int chunk = GSR_XCD_DEPTH && ITEMS == 16 ? xcd_chunk((int)blockIdx.x, groups) : (int)blockIdx.x;
    chunk_range(n, groups, chunk, kTile, b, e);

    // global base of each digit for this workgroup (a filtered pass 0: the kept count is
    // the sum of the digit totals)
    uint32_t gb;   // digit t's running global offset (thread t owns digit t)
    {
        uint32_t tot;
        const uint32_t dig_excl = block_exclusive_scan<uint32_t>(totals[t], s_scr, tot);
        gb = dig_excl + hist[t * (uint32_t)groups + chunk];
        if (FILT && sr.count_out && blockIdx.x == 0 && t == 0) *sr.count_out = tot;
    }
    if (b >= e) return;                          // uniform per workgroup
    const uint64_t lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));

    for (uint64_t tb = b; tb < e; tb += kTile) {
        const uint32_t tn = (uint32_t)min((uint64_t)kTile, e - tb);
#pragma unroll
        for (int k = 0; k < 4; k++) s_wc[k][t] = 0;
        __syncthreads();

        uint64_t it[ITEMS];
        uint32_t rk[ITEMS], pv[ITEMS];
        bool kp[ITEMS];   // in the tile and kept (a filtered pass 0 drops the other part)
        const uint32_t wbase = w * 64 * ITEMS;
        // tile-relative 32-bit offsets from a uniform base: one address VGPR for all ITEMS
        // loads (64-bit per-item addresses had the 16-item kernel at 164+ VGPRs)
        const uint64_t* __restrict__ in_t = in + tb;
#pragma unroll
        for (int k = 0; k < ITEMS; k++) {
            const uint32_t el = wbase + k * 64 + lane;
            it[k] = (el < tn) ? in_t[el] : 0ull;
        }
        auto load_pay = [&]() {
            if (!carry) return;
            // uniform branches: the position-indexed reads must not wait for the item loads
            const uint32_t* src = (pay_in ? pay_in : rect) + tb;
            if (pay_in || rect_direct) {
#pragma unroll
                for (int k = 0; k < ITEMS; k++) {
                    const uint32_t el = wbase + k * 64 + lane;
                    pv[k] = (el < tn) ? src[el] : 0u;
                }
            } else {
#pragma unroll
                for (int k = 0; k < ITEMS; k++) {
                    const uint32_t el = wbase + k * 64 + lane;
                    pv[k] = (el < tn) ? rect[(uint32_t)it[k]] : 0u;
                }
            }
        };
        // a filtered pass 0 ranks by the payloads; otherwise they are loaded after the
        // ranking (their latency hides behind the tile scan, and the ranking holds 16 fewer
        // VGPRs at 16 items per thread)
        if (FILT) load_pay();
        uint32_t before[ITEMS];
#pragma unroll
        for (int k = 0; k < ITEMS; k++) {
            const uint32_t el = wbase + k * 64 + lane;
            const bool valid = el < tn && (!FILT || sort_keep(sr, K, it[k], pv[k]));
            kp[k] = valid;
            const uint32_t d = (uint32_t)(it[k] >> shift) & mask;
            // returning atomics at 4-8 items per thread; at 16 (4M+ items) ballot matching
            if (RA && ITEMS < 16) {
                rk[k] = valid ? atomicAdd(&s_wc[w][d], 1u) : 0u;
                before[k] = 0;
            } else {
                // every lane reads its digit's running count and the digit's leader adds the
                // slot's count without a return: a wave's LDS ops execute in issue order, so
                // slot k's read sees slots < k and no read is waited on before the next slot
                // (reading, waiting and writing back per slot serialised 16 LDS round trips)
                // (digits of fewer than 8 bits are masked: their high ballots match all)
                const uint64_t peers = match_peers<8>(d, valid, 8);
                rk[k] = (uint32_t)__popcll(peers & lt_mask);
                before[k] = s_wc[w][d];
                if (valid && (uint32_t)(__ffsll((unsigned long long)peers) - 1) == lane)
                    atomicAdd(&s_wc[w][d], (uint32_t)__popcll(peers));
                // the reads fold into the ranks every 4 slots (the compiler places the waits
                // for them; the VGPR peak came from hoisted loop invariants, see below)
                if ((k & 3) == 3)
#pragma unroll
                    for (int j = k - 3; j <= k; j++) rk[j] += before[j];
            }
        }
        if (!FILT) load_pay();
        __syncthreads();
        // per digit t: tile count, tile-local base, and each wave's first slot (tile base
        // included, so an item reads one word for its slot); the write-back's base is kept
        // as global offset minus tile slot (one word per item there too)
        uint32_t tcount, tv;   // tv: the tile's kept items (tn unless filtered)
        {
            const uint32_t c0 = s_wc[0][t], c1 = s_wc[1][t], c2 = s_wc[2][t], c3 = s_wc[3][t];
            tcount = c0 + c1 + c2 + c3;
            const uint32_t lb = block_exclusive_scan<uint32_t>(tcount, s_scr, tv);   // barriers: reads done
            s_wc[0][t] = lb;
            s_wc[1][t] = lb + c0;
            s_wc[2][t] = lb + c0 + c1;
            s_wc[3][t] = lb + c0 + c1 + c2;
            s_gd[t] = gb - lb;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < ITEMS; k++) {
            if (kp[k]) {
                const uint32_t d = (uint32_t)(it[k] >> shift) & mask;
                const uint32_t slot = s_wc[w][d] + rk[k];
                s_items[slot] = it[k];
                if (kPaySlots && carry) s_payd[slot] = pv[k];
                rk[k] = slot;   // the payload round's slot (the items die here)
            }
        }
        __syncthreads();
        // the digits of the items this thread wrote, four per word: the payload round
        // rebuilds their destinations from them (16 destinations held across the round
        // took the 16-item kernel to 179 VGPRs, two workgroups per CU)
        uint32_t dpk[(ITEMS + 3) / 4];
#pragma unroll
        for (int k = 0; k < (ITEMS + 3) / 4; k++) dpk[k] = 0;
#pragma unroll
        for (int k = 0; k < ITEMS; k++) {
            const uint32_t q = t + k * kSortThreads;
            if (q < tv) {
                const uint64_t v = s_items[q];
                const uint32_t d = (uint32_t)(v >> shift) & mask;
                const uint32_t dst = s_gd[d] + q;
                out[dst] = v;
                if (kPaySlots && carry) pay_out[dst] = s_payd[q];
                dpk[k / 4] |= d << (8 * (k % 4));
                if (ranges) {
                    // final pass of the tile sort: the LDS tile is fully sorted, so each
                    // run of one tile key is contiguous; record its global [start, end)
                    // as {~start, end} with atomicMax, so a zeroed array means "empty"
                    // (replaces a separate boundary-detection kernel).
                    const uint32_t key = (uint32_t)(v >> 32);
                    if (q == 0 || (uint32_t)(s_items[q - 1] >> 32) != key) atomicMax(&ranges[key].x, ~dst);
                    if (q == tv - 1 || (uint32_t)(s_items[q + 1] >> 32) != key) atomicMax(&ranges[key].y, dst + 1);
                }
            }
        }
        if (!kPaySlots && carry) {
            // the payloads take the items' LDS slots once every item is read, so their
            // stores leave in the same digit runs as the items' (coalesced)
            uint32_t* s_pay = reinterpret_cast<uint32_t*>(s_items);
            __syncthreads();
#pragma unroll
            for (int k = 0; k < ITEMS; k++)
                if (kp[k]) s_pay[rk[k]] = pv[k];
            __syncthreads();
#pragma unroll
            for (int k = 0; k < ITEMS; k++) {
                const uint32_t q = t + k * kSortThreads;
                const uint32_t d = (dpk[k / 4] >> (8 * (k % 4))) & 0xffu;
                if (q < tv) pay_out[s_gd[d] + q] = s_pay[q];
            }
        }
        // 16 items per thread: one tile per workgroup (launch_radix_pass checks the grid),
        // so the loop is straight-line code and nothing is hoisted across tiles (the
        // loop-invariant slot offsets of the write-back held 15 VGPRs for the whole kernel)
        if (ITEMS == 16) break;
        __syncthreads();   // every read of s_gd / s_wc done before the next tile's writes
        gb += tcount;
    }
}

// Key-value variant for the tile sort: keys of type K (uint16_t when the frame
// has <= 65536 tiles, else uint32_t) and uint32_t values in separate arrays,
// so the upsweep reads only the keys and the final pass writes only the values
// (plus the tile ranges).  Same reduce-then-scan structure and ranking.
template <typename K, int ITEMS>
__global__ __launch_bounds__(kSortThreads) void k_kv_upsweep(const K* __restrict__ keys,
                                                             const uint32_t* __restrict__ n_dev, int shift,
                                                             uint32_t mask, int groups,
                                                             uint32_t* __restrict__ hist) {
    GSR_GEOM_PRIO();
    __shared__ uint32_t h[4][256];
    const uint32_t t = threadIdx.x;
    const uint32_t w = t >> 6;
#pragma unroll
    for (int k = 0; k < 4; k++) h[k][t] = 0;
    __syncthreads();
    const uint64_t n = (uint64_t)*n_dev;
    uint64_t b, e;
    chunk_range(n, groups, blockIdx.x, kSortThreads * ITEMS, b, e);
    uint64_t i = b + t;
    for (; i + 3 * kSortThreads < e; i += 4 * kSortThreads) {
        const uint32_t k0 = keys[i], k1 = keys[i + kSortThreads], k2 = keys[i + 2 * kSortThreads],
                       k3 = keys[i + 3 * kSortThreads];
        atomicAdd(&h[w][(k0 >> shift) & mask], 1u);
        atomicAdd(&h[w][(k1 >> shift) & mask], 1u);
        atomicAdd(&h[w][(k2 >> shift) & mask], 1u);
        atomicAdd(&h[w][(k3 >> shift) & mask], 1u);
    }
    for (; i < e; i += kSortThreads) atomicAdd(&h[w][((uint32_t)keys[i] >> shift) & mask], 1u);
    __syncthreads();
    hist[t * (uint32_t)groups + blockIdx.x] = h[0][t] + h[1][t] + h[2][t] + h[3][t];
}

// keys_out == nullptr: final pass — write values only and record each tile's
// global [start, end) as {~start, end} (atomicMax; a zeroed array = empty).
template <typename K, int ITEMS>
__global__ __launch_bounds__(kSortThreads) void k_kv_downsweep(
    const K* __restrict__ keys_in, const uint32_t* __restrict__ vals_in, K* __restrict__ keys_out,
    uint32_t* __restrict__ vals_out, const uint32_t* __restrict__ n_dev, int shift, int bits, int groups,
    const uint32_t* __restrict__ hist, const uint32_t* __restrict__ totals, uint2* __restrict__ ranges) {
    GSR_GEOM_PRIO();
    constexpr int kTile = kSortThreads * ITEMS;
    __shared__ K s_keys[kTile];
    __shared__ uint32_t s_vals[kTile];
    __shared__ uint32_t s_wc[4][256];
    __shared__ uint32_t s_gbase[256];
    __shared__ uint32_t s_lbase[256];
    __shared__ uint32_t s_scr[4];
    const uint32_t t = threadIdx.x;
    const uint32_t lane = lane_id();
    const uint32_t w = t >> 6;
    const uint32_t mask = (1u << bits) - 1u;
    const uint64_t n = (uint64_t)*n_dev;
    uint64_t b, e;
    chunk_range(n, groups, blockIdx.x, kTile, b, e);
    if (b >= e) return;
    {
        uint32_t tot;
        const uint32_t dig_excl = block_exclusive_scan<uint32_t>(totals[t], s_scr, tot);
        s_gbase[t] = dig_excl + hist[t * (uint32_t)groups + blockIdx.x];
    }
    const uint64_t lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));

    for (uint64_t tb = b; tb < e; tb += kTile) {
        const uint32_t tn = (uint32_t)min((uint64_t)kTile, e - tb);
#pragma unroll
        for (int k = 0; k < 4; k++) s_wc[k][t] = 0;
        __syncthreads();
        uint32_t kk[ITEMS], vv[ITEMS], rk[ITEMS];
        const uint32_t wbase = w * 64 * ITEMS;
#pragma unroll
        for (int k = 0; k < ITEMS; k++) {
            const uint32_t el = wbase + k * 64 + lane;
            kk[k] = (el < tn) ? (uint32_t)keys_in[tb + el] : 0u;
            vv[k] = (el < tn) ? vals_in[tb + el] : 0u;
        }
#pragma unroll
        for (int k = 0; k < ITEMS; k++) {
            const uint32_t el = wbase + k * 64 + lane;
            const bool valid = el < tn;
            const uint32_t d = (kk[k] >> shift) & mask;
            const uint64_t peers = match_peers<8>(d, valid, bits);
            uint32_t r = 0;
            if (valid) {
                const uint32_t before = s_wc[w][d];
                r = before + (uint32_t)__popcll(peers & lt_mask);
                if ((uint32_t)(__ffsll((unsigned long long)peers) - 1) == lane)
                    s_wc[w][d] = before + (uint32_t)__popcll(peers);
            }
            rk[k] = r;
        }
        __syncthreads();
        uint32_t tcount;
        {
            const uint32_t c0 = s_wc[0][t], c1 = s_wc[1][t], c2 = s_wc[2][t], c3 = s_wc[3][t];
            s_wc[0][t] = 0;
            s_wc[1][t] = c0;
            s_wc[2][t] = c0 + c1;
            s_wc[3][t] = c0 + c1 + c2;
            tcount = c0 + c1 + c2 + c3;
            uint32_t tot;
            s_lbase[t] = block_exclusive_scan<uint32_t>(tcount, s_scr, tot);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < ITEMS; k++) {
            const uint32_t el = wbase + k * 64 + lane;
            if (el < tn) {
                const uint32_t d = (kk[k] >> shift) & mask;
                const uint32_t q = s_lbase[d] + s_wc[w][d] + rk[k];
                s_keys[q] = (K)kk[k];
                s_vals[q] = vv[k];
            }
        }
        __syncthreads();
        for (uint32_t q = t; q < tn; q += kSortThreads) {
            const uint32_t key = s_keys[q];
            const uint32_t d = (key >> shift) & mask;
            const uint32_t dst = s_gbase[d] + (q - s_lbase[d]);
            vals_out[dst] = s_vals[q];
            if (keys_out) {
                keys_out[dst] = (K)key;
            } else {
                if (q == 0 || (uint32_t)s_keys[q - 1] != key) atomicMax(&ranges[key].x, ~dst);
                if (q == tn - 1 || (uint32_t)s_keys[q + 1] != key) atomicMax(&ranges[key].y, dst + 1);
            }
        }
        __syncthreads();
        s_gbase[t] += tcount;
    }
}

// ------------------------------------------------------------------ emission

// Tile counts in depth order.  The one random access of the emission — the
// compact rect of Gaussian sorted[j] — happens here, once; the rects are
// written back in depth order (srect) so k_emit_pairs reads them coalesced.
// Each thread issues all four of its index loads, then all four rect gathers,
// so the dependent gathers overlap instead of running back to back.
// The depth sort ends in items[passes run & 1] (depth_sorted); the other buffer is free
// for srect.
// The depth-ordered rect payloads the binning's depth sort carries (k_radix_downsweep):
// same parity as the items.
__device__ __forceinline__ const uint32_t* depth_sorted_rects(const uint32_t* pay0, const uint32_t* pay1,
                                                             const uint32_t* dstats) {
    return (depth_passes_run(dstats) & 1) ? pay1 : pay0;
}

__global__ __launch_bounds__(256) void k_emit_count(const uint64_t* __restrict__ items0,
                                                     const uint64_t* __restrict__ items1,
                                                     const uint32_t* __restrict__ dstats, uint32_t n,
                                                     const uint64_t* __restrict__ rect, int groups,
                                                     unsigned long long* __restrict__ wg_sum,
                                                     uint2* __restrict__ ranges, int ntiles) {
    GSR_GEOM_PRIO();
    __shared__ unsigned long long scr[4];
    // zero the tile ranges for the tile sort's final pass (a slice per workgroup)
    for (int q = blockIdx.x * 256 + threadIdx.x; q < ntiles; q += groups * 256) ranges[q] = make_uint2(0u, 0u);
    const uint64_t* sorted = depth_sorted(items0, items1, dstats);
    uint64_t* srect = const_cast<uint64_t*>(sorted == items0 ? items1 : items0);
    uint64_t b, e;
    chunk_range(n, groups, blockIdx.x, 1024, b, e);
    unsigned long long s = 0;
    for (uint64_t c0 = b; c0 < e; c0 += 1024) {
        uint32_t gi[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint64_t j = c0 + threadIdx.x + 256 * k;
            gi[k] = j < e ? (uint32_t)sorted[j] : 0u;
        }
        uint64_t r[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint64_t j = c0 + threadIdx.x + 256 * k;
            r[k] = j < e ? rect[gi[k]] : kDeadRect;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint64_t j = c0 + threadIdx.x + 256 * k;
            if (j < e) srect[j] = r[k];
            s += rect_count(r[k]);
        }
    }
    unsigned long long tot;
    block_exclusive_scan<unsigned long long>(s, scr, tot);
    if (threadIdx.x == 0) wg_sum[blockIdx.x] = tot;
}

// Exclusive scan of the per-workgroup pair counts + the frame's pair stats.
// (Folding it into k_emit_count's last-arriving workgroup was measured slower:
// the agent-scope fences before each arrival ticket write back the L2 on gfx950.)
__global__ __launch_bounds__(256) void k_emit_scan(unsigned long long* __restrict__ wg, int groups,
                                                    uint32_t cap, Stats* __restrict__ st,
                                                    Stats* host_st, uint32_t* fstatus) {
    GSR_GEOM_PRIO();
    __shared__ unsigned long long scr[4];
    const int per = (groups + 255) / 256;
    const int b = threadIdx.x * per;
    unsigned long long local = 0;
    for (int k = 0; k < per; k++)
        if (b + k < groups) local += wg[b + k];
    unsigned long long total;
    unsigned long long run = block_exclusive_scan<unsigned long long>(local, scr, total);
    for (int k = 0; k < per; k++)
        if (b + k < groups) {
            const unsigned long long v = wg[b + k];
            wg[b + k] = run;
            run += v;
        }
    if (threadIdx.x == 0) {
        Stats s{};
        s.pairs_total = total;
        s.pairs_eff = (uint32_t)(total < cap ? total : cap);
        s.overflow = total > cap ? 1u : 0u;
        st[0] = s;
        // st[1]: sticky record (max P, overflow seen) until the host clears it
        Stats k = st[1];
        if (s.pairs_total > k.pairs_total) k.pairs_total = s.pairs_total;
        k.pairs_eff = s.pairs_eff;
        k.overflow |= s.overflow;
        st[1] = k;
        if (fstatus) *fstatus = s.overflow;
        if (host_st) {
            host_st->pairs_total = k.pairs_total;
            host_st->pairs_eff = k.pairs_eff;
            host_st->overflow = k.overflow;
            __threadfence_system();
        }
    }
}

// One (tile key, Gaussian index) pair per covered tile, in depth order, as
// separate key (K = uint16_t or uint32_t) and value (uint32_t) arrays for the
// key-value tile sort [render.cu:788-809].  Each wave owns 256 consecutive
// Gaussians of the workgroup's 1024 and writes their pairs cooperatively:
// per round of 64 Gaussians, lane l of a 64-pair step finds its Gaussian by a
// binary search over the round's inclusive count prefix, so every store
// instruction writes 64 consecutive pairs.
template <typename K>
__global__ __launch_bounds__(256) void k_emit_pairs(const uint64_t* __restrict__ items0,
                                                     const uint64_t* __restrict__ items1,
                                                     const uint32_t* __restrict__ dstats, uint32_t n, int groups,
                                                     const unsigned long long* __restrict__ wg_base,
                                                     uint32_t cap, int tiles_x, K* __restrict__ keys,
                                                     uint32_t* __restrict__ vals) {
    GSR_GEOM_PRIO();
    __shared__ unsigned long long scr[4];
    __shared__ uint32_t s_incl[4][64], s_idx[4][64];
    __shared__ uint64_t s_rect[4][64];
    const uint64_t* sorted = depth_sorted(items0, items1, dstats);
    const uint64_t* srect = sorted == items0 ? items1 : items0;
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    uint64_t b, e;
    chunk_range(n, groups, blockIdx.x, 1024, b, e);
    unsigned long long run = wg_base[blockIdx.x];
    for (uint64_t c0 = b; c0 < e; c0 += 1024) {
        // this wave's 256 Gaussians: [c0 + 256 w, +256), four rounds of 64
        uint32_t cnt[4], gi[4];
        uint64_t r[4];
        uint32_t wtot = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint64_t j = c0 + 256 * w + 64 * k + lane;
            gi[k] = j < e ? (uint32_t)sorted[j] : 0u;
            r[k] = j < e ? srect[j] : kDeadRect;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            cnt[k] = rect_count(r[k]);
            wtot += cnt[k];
        }
        // wave totals -> exclusive base of this wave inside the 1024-chunk
        unsigned long long chunk_tot;
        const unsigned long long wsum = (unsigned long long)__reduce_add_sync(~0ull, wtot);
        const unsigned long long wbase = block_exclusive_scan<unsigned long long>(lane == 0 ? wsum : 0ull, scr,
                                                                                  chunk_tot);
        unsigned long long pos = run + (unsigned long long)__shfl(wbase, 0, 64);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            // inclusive prefix of the round's counts
            const uint32_t incl = wave_incl_scan(cnt[k], OpAdd{});
            const uint32_t rtot = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            s_incl[w][lane] = incl;
            s_idx[w][lane] = gi[k];
            s_rect[w][lane] = r[k];
            for (uint32_t q = lane; q < rtot; q += 64) {
                // Gaussian l: the first lane whose inclusive prefix exceeds q
                uint32_t l = 0;
#pragma unroll
                for (uint32_t st = 32; st >= 1; st >>= 1)
                    if (s_incl[w][l + st - 1] <= q) l += st;
                const uint64_t rr = s_rect[w][l];
                const uint32_t before = s_incl[w][l] - rect_count(rr);   // exclusive prefix of Gaussian l
                const uint32_t k2 = q - before;
                const uint32_t tx0 = (uint32_t)(rr & 0xffffu), tx1 = (uint32_t)((rr >> 16) & 0xffffu);
                const uint32_t ty0 = (uint32_t)((rr >> 32) & 0xffffu);
                const uint32_t wdt = tx1 - tx0 + 1u;
                const uint32_t dy = k2 / wdt, dx = k2 - dy * wdt;
                const unsigned long long p = pos + q;
                if (p < cap) {
                    keys[p] = (K)((ty0 + dy) * (uint32_t)tiles_x + tx0 + dx);
                    vals[p] = s_idx[w][l];
                }
            }
            pos += rtot;
        }
        run += chunk_tot;
    }
}

// ------------------------------------------------------------------ tile binning
//
// For tile grids up to 256 x 256, two stable counting passes replace "emit every
// (tile, Gaussian) pair in depth order, then LSD-sort the pairs by tile":
//   row pass     each depth-ordered Gaussian expands into one item per covered
//                tile ROW (index | tx0 << 32 | tx1 << 48), binned stably by row:
//                ~2.4 items per Gaussian instead of ~5.6 pairs
//   column pass  each row's items expand into one value per covered tile COLUMN,
//                binned stably by column inside the row: the final tile-major,
//                depth-ordered Gaussian indices; the tile ranges come straight
//                from the column scan and no tile key is ever stored
// Each pass is count (per-chunk histograms) -> scan -> scatter.  The scatters
// rank one tile of generated items at a time in LDS (wave ballots on the digit
// bits) and write them digit run by digit run, so the stores coalesce.  Every
// source is processed in order and chunks are scanned in order: the result is
// the same stable order as the pair sort [render.cu:788-857].

constexpr uint32_t kRowSources = 1024;              // Gaussians per row-pass sub-chunk
// Row items per column-pass chunk (a chunk never crosses a row): 1,024 or 2,048, chosen
// per frame by the runtime (GSR_TUNE_COL_CHUNK).  Smaller chunks halve the scatter's
// per-chunk LDS (config 2: column scatter 26.0 -> 21.6 us); on config 3's ~9M row items
// the doubled chunk count costs the count and scan more (+10 us), so 2,048 stays there
// (profiles/r05_ab_col_chunk.txt).
constexpr uint32_t kColChunkMin = 1024, kColChunkMax = 2048;

__device__ __forceinline__ uint32_t rect_rows(uint64_t r) {
    return rect_count(r) ? (uint32_t)((r >> 48) - ((r >> 32) & 0xffffu) + 1u) : 0u;
}
__device__ __forceinline__ uint32_t rect_cols(uint64_t r) {
    return rect_count(r) ? (uint32_t)(((r >> 16) & 0xffffu) - (r & 0xffffu) + 1u) : 0u;
}

// Stable rank of one tile of up to 256*ITEMS items with BITS-bit digits.  Item
// k of thread t is tile element w*64*ITEMS + k*64 + lane (each wave's items are
// contiguous).  On return pos[k] is the item's slot in the digit-sorted tile,
// s_lbase[d] the first slot of digit d; returns the tile's count of digit t.
// Per k-slot every lane reads its digit's running wave count and the slot's
// leader of each digit ADDS the slot's count (ds_add, no return): LDS ops of a
// wave execute in issue order, so slot k's read sees slots < k and nothing waits
// on a read before the next slot is issued.
template <int ITEMS, int BITS, bool RA>
__device__ __forceinline__ uint32_t bin_rank_tile(const uint32_t (&dig)[ITEMS], uint32_t tn,
                                                  uint32_t (&pos)[ITEMS], uint32_t (*s_wc)[256],
                                                  uint32_t* s_lbase, uint32_t* s_scr) {
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    const uint64_t lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
#pragma unroll
    for (int k = 0; k < 4; k++) s_wc[k][t] = 0;
    __syncthreads();
    if (RA) {
#pragma unroll
        for (int k = 0; k < ITEMS; k++) {
            const uint32_t el = w * 64 * ITEMS + k * 64 + lane;
            pos[k] = el < tn ? atomicAdd(&s_wc[w][dig[k]], 1u) : 0u;
        }
    } else {
        uint32_t before[ITEMS], inslot[ITEMS];
#pragma unroll
        for (int k = 0; k < ITEMS; k++) {
            const uint32_t el = w * 64 * ITEMS + k * 64 + lane;
            const bool valid = el < tn;
            const uint32_t d = dig[k];
            const uint64_t peers = match_peers<BITS>(d, valid, BITS);
            inslot[k] = (uint32_t)__popcll(peers & lt_mask);
            before[k] = s_wc[w][d];
            if (valid && (uint32_t)(__ffsll((unsigned long long)peers) - 1) == lane)
                atomicAdd(&s_wc[w][d], (uint32_t)__popcll(peers));
        }
#pragma unroll
        for (int k = 0; k < ITEMS; k++) pos[k] = before[k] + inslot[k];
    }
    __syncthreads();
    uint32_t tcount;
    {
        // each wave's first slot of digit t, tile base included (s_wc[w][t] = s_lbase[t] +
        // the earlier waves' counts), so an item reads one word for its slot, not two
        const uint32_t c0 = s_wc[0][t], c1 = s_wc[1][t], c2 = s_wc[2][t], c3 = s_wc[3][t];
        tcount = c0 + c1 + c2 + c3;
        uint32_t tot;
        const uint32_t lb = block_exclusive_scan<uint32_t>(tcount, s_scr, tot);   // barriers: reads done
        s_lbase[t] = lb;
        s_wc[0][t] = lb;
        s_wc[1][t] = lb + c0;
        s_wc[2][t] = lb + c0 + c1;
        s_wc[3][t] = lb + c0 + c1 + c2;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < ITEMS; k++) {
        const uint32_t el = w * 64 * ITEMS + k * 64 + lane;
        if (el < tn) pos[k] += s_wc[w][dig[k]];
    }
    return tcount;
}

// Exclusive starts (in source order) of per-source counts cnt[] (thread t owns sources
// PER*t .. PER*t + PER-1): returns them in start[] and the total, and writes each with
// an 8-bit tag (the source's first row or column) to s_ft[s] = start << 8 | tag, so an
// element reads one word for both (starts stay below 2^24: <= 2,048 sources x 256
// digits).  Two barriers.
template <int PER>
__device__ __forceinline__ uint32_t bin_source_starts(const uint32_t (&cnt)[PER], uint32_t (&start)[PER],
                                                      const uint32_t (&tag)[PER], uint32_t* s_ft, uint32_t* s_scr) {
    const uint32_t t = threadIdx.x;
    uint32_t loc = 0;
#pragma unroll
    for (int i = 0; i < PER; i++) loc += cnt[i];
    uint32_t tot;
    uint32_t run = block_exclusive_scan<uint32_t>(loc, s_scr, tot);
#pragma unroll
    for (int i = 0; i < PER; i++) {
        start[i] = run;
        s_ft[PER * t + i] = (run << 8) | tag[i];
        run += cnt[i];
    }
    return tot;
}

// Source of every element of the tile [tb, tb + tn) of a generated stream,
// without a per-element search: each source starting inside the tile marks its
// first element (slot + 1) in s_own (cleared beforehand), then an in-order
// inclusive max-scan fills the runs.  `carry` (slot + 1 owning the element
// before the tile; 0 at a stream's start) seeds the scan and becomes the owner
// of the tile's last element.  The scan runs thread-major inside each wave
// (lane handles elements w*64*ITEMS + lane*ITEMS + i), so every wave scans its
// own ITEMS*64 elements in order.  Three barriers.
template <int ITEMS, int PER>
__device__ __forceinline__ void bin_tile_owners(const uint32_t (&cnt)[PER], const uint32_t (&start)[PER],
                                                uint32_t tb, uint32_t tn, uint16_t* s_own, uint32_t& carry,
                                                uint32_t* s_wmax) {
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
#pragma unroll
    for (int i = 0; i < PER; i++)
        if (cnt[i] && start[i] >= tb && start[i] < tb + tn) s_own[start[i] - tb] = (uint16_t)(PER * t + i + 1);
    __syncthreads();
    const uint32_t base = w * 64 * ITEMS + lane * ITEMS;
    uint32_t v[ITEMS], run = 0;
#pragma unroll
    for (int i = 0; i < ITEMS; i++) {
        run = max(run, (uint32_t)s_own[base + i]);
        v[i] = run;
    }
    // exclusive max over the earlier lanes of the wave, then over earlier waves
    const uint32_t x = wave_incl_scan(run, OpMax{});
    if (lane == 63) s_wmax[w] = x;
    const uint32_t before = wave_shr1(x);
    __syncthreads();
    uint32_t cin = carry;
    for (uint32_t k = 0; k < w; k++) cin = max(cin, s_wmax[k]);
    cin = max(cin, before);
#pragma unroll
    for (int i = 0; i < ITEMS; i++) s_own[base + i] = (uint16_t)max(cin, v[i]);
    carry = max(max(carry, max(s_wmax[0], s_wmax[1])), max(s_wmax[2], s_wmax[3]));
    __syncthreads();
}

// Frame pair statistics (st[0]) + the sticky copy (st[1], and the host-mapped
// mirror) the non-blocking overflow check reads.
// Binning path: `needed` = depth passes the device plan asked for, `launched` = passes
// the host launched (its pass budget); needed > launched leaves the depth order
// incomplete, so the frame is flagged (overflow bit 1) and re-rendered like a
// pair-buffer overflow.  depth_passes is the latest frame's, not sticky.
// fstatus (nullable): the frame's validity word (gsr_render_path_status): set to the
// frame's overflow bits by its first column scan (fst_first: phase A or one phase),
// or-ed in by phase B's.
__device__ __forceinline__ void publish_pair_stats(unsigned long long total, uint32_t cap, Stats* st,
                                                   Stats* host_st, uint32_t needed = 0, uint32_t launched = 4,
                                                   uint32_t* fstatus = nullptr, bool fst_first = true) {
    Stats s{};
    s.pairs_total = total;
    s.pairs_eff = (uint32_t)(total < cap ? total : cap);
    s.overflow = (total > cap ? 1u : 0u) | (needed > launched ? 2u : 0u);
    s.depth_passes = needed;
    st[0] = s;
    Stats k = st[1];
    if (s.pairs_total > k.pairs_total) k.pairs_total = s.pairs_total;
    k.pairs_eff = s.pairs_eff;
    k.overflow |= s.overflow;
    k.depth_passes = s.depth_passes;
    st[1] = k;
    if (fstatus) {
        if (fst_first) *fstatus = s.overflow;
        else if (s.overflow) atomicOr(fstatus, s.overflow);
    }
    if (host_st) {
        host_st->pairs_total = k.pairs_total;
        host_st->pairs_eff = k.pairs_eff;
        host_st->overflow = k.overflow;
        host_st->depth_passes = k.depth_passes;
        __threadfence_system();
    }
}

// Depth-order positions a row pass reads: [base, base + n) as the host passed them, or
// with the depth split's device-side cut (the near part's size after the threshold
// partition): mode 1 = [0, min(cut, n)) (phase A), mode 2 = [cut, n) (phase B).
// (mode 2 with cut_n: the far part's kept length *cut_n, a masked far sort's count.)
__device__ __forceinline__ void row_range(uint32_t& base, uint32_t& n, const uint32_t* cut, int mode,
                                          const uint32_t* cut_n) {
    if (mode == 1) {
        n = min(*cut, n);
    } else if (mode == 2) {
        base = min(*cut, n);
        n -= base;
        if (cut_n) n = min(*cut_n, n);
    }
}

// ------------------------------------------------------------------ bucket depth sort
//
// The binning path's global depth sort in two global steps instead of three or four
// LSD passes (GSR_TUNE_DEPTH_BUCKETS).  Stable order of (depth key, index), exactly
// the LSD passes' order:
//   k_bkt_count    per workgroup chunk, the histogram over B buckets: bucket(key) =
//                  the number of splitters <= key (B - 1 sorted splitters in LDS; the
//                  last is 0xFFFFFFFF, so bucket B - 1 holds exactly the keys equal to
//                  0xFFFFFFFF: culled items and saturated live keys, which tie)
//   k_bkt_scan     per bucket, exclusive scan over the chunks (a chunk-major histogram:
//                  every access a coalesced row segment); k_bkt_scan_g for the big kind
//   k_bkt_scatter  stable scatter of the preprocess order into the buckets (per-wave
//                  returning LDS atomics on packed 16-bit counters, so the rank of an
//                  item is its order among the wave's earlier items of its bucket);
//                  every item lands at its bucket's range, index-ordered inside it; the
//                  tile rects ride along as payloads
//   k_bkt_local    one workgroup per live bucket: load it (<= kBktCap items), stable
//                  LSD in LDS over the bits (key - bucket min) spans (typically 11 on
//                  config 2: two 8-bit passes), write it back in place.  A bucket over
//                  capacity is sorted by the same workgroup through global memory
//                  (stable 8-bit passes ping-ponging with the scratch buffer), so any
//                  splitters give the exact order; they only set the speed
// Two kinds ship (gsr_runtime.cpp bkt_big).  Small (up to 2M items, B = 256..4,096 by size):
// k_bkt_count, k_bkt_scan, the unstaged k_bkt_scatter (16-B records, its own splitter search),
// k_bkt_local.  Big (above 2M, B = kBigBuckets): k_bkt_count handing each item's bucket on,
// k_bkt_scan_g, the staged k_bkt_scatter (12-B records), k_bbk_local, then k_bkt_local for the
// buckets k_bbk_local left.
// Splitters are the previous frame's quantiles: k_bkt_local writes the key at each
// bkt_split_pos of the live order for the next frame (double-buffered; the open first and
// last live buckets a quarter share, the rest even), so the buckets hold about n / B
// items each while the camera moves smoothly.  A context's
// first frame runs the LSD passes and k_bkt_splitters takes the quantiles from them.
// Stability: the scatter keeps index order inside a bucket, the local passes are stable
// and buckets are key ranges in order, so ties stay in index order — the same order as
// render.cu's CUB SortPairs of (tile << 32 | depth) within each tile (render.cu:1099-1118).
constexpr int kBktThreads = 256;
constexpr int kBktItems = 8;                                  // items per thread per tile
constexpr uint32_t kBktTile = kBktThreads * kBktItems;        // 2048
constexpr uint32_t kBktCap = kBktTile;                        // local sort capacity (items)
static_assert(kBktCap == kMaxBucketCap && kMaxBuckets == 4096, "gsr_internal.h bucket sort limits");

// The splitters in LDS as an implicit search tree in breadth-first (Eytzinger) order:
// node i at depth d, position p = i + 1 - 2^d holds the sorted splitter of rank
// (2p + 1) 2^(h - 1 - d) - 1 (h = log2 B; the B - 1 splitters fill the tree exactly).  Each
// search step reads one tree level, and a level's nodes are consecutive words.  (The plain
// sorted array put every address of the first search steps on ONE LDS bank -- b + st - 1
// with b a multiple of 2 st -- up to 32-way conflicts: the count kernel took 10 us.)
template <int B, int TH = kBktThreads>
__device__ __forceinline__ void bkt_load_splitters(uint32_t* s_T, const uint32_t* __restrict__ splitters) {
    // B / TH nodes per thread, every load issued before the first LDS write: a rolled
    // loop waited for each load in turn (four serial memory round trips at B = 1,024)
    static_assert(B >= TH, "one node per thread at least");
    constexpr int h = __builtin_ctz(B);
    constexpr int kPer = B / TH;
    uint32_t v[kPer], jj[kPer];
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const uint32_t i = threadIdx.x + (uint32_t)k * TH;
        const int d = 31 - __clz((int)(i + 1u));
        const uint32_t p = i + 1u - (1u << d);
        const int sh = h - 1 - d;                               // < 0 only for i = B - 1 (no node)
        jj[k] = sh >= 0 ? ((2u * p + 1u) << sh) - 1u : (uint32_t)B - 2u;   // sorted rank
        v[k] = splitters[min(jj[k], (uint32_t)B - 3u)];
    }
#pragma unroll
    for (int k = 0; k < kPer; k++)
        s_T[threadIdx.x + (uint32_t)k * TH] = jj[k] < (uint32_t)B - 2u ? v[k] : 0xffffffffu;
}

// The buckets of N keys: bucket(key) = the number of the B - 1 sorted splitters that are
// <= key (the last is 0xFFFFFFFF, so a key 0xFFFFFFFF lands in bucket B - 1), by a walk
// down the tree of bkt_load_splitters.  Level by level, so each level's N LDS reads are in
// flight together.
template <int B, int N>
__device__ __forceinline__ void bkt_of_n(const uint32_t* s_T, const uint32_t (&key)[N], uint32_t (&bk)[N]) {
#pragma unroll
    for (int k = 0; k < N; k++) bk[k] = 0;
#pragma unroll
    for (int lvl = 0; lvl < __builtin_ctz(B); lvl++) {
        uint32_t v[N];
#pragma unroll
        for (int k = 0; k < N; k++) v[k] = s_T[bk[k]];
#pragma unroll
        for (int k = 0; k < N; k++) bk[k] = 2u * bk[k] + (v[k] <= key[k] ? 2u : 1u);
    }
#pragma unroll
    for (int k = 0; k < N; k++) bk[k] -= (uint32_t)B - 1u;
}

template <int B>
__global__ __launch_bounds__(kBktThreads) void k_bkt_count(const uint64_t* __restrict__ in, uint32_t n,
                                                           const uint32_t* __restrict__ splitters, int groups,
                                                           uint32_t* __restrict__ hist,
                                                           uint16_t* __restrict__ bid = nullptr) {
    GSR_GEOM_PRIO();
    __shared__ uint32_t s_S[B], s_h[B];
    const uint32_t t = threadIdx.x, lane = t & 63u;
    uint64_t b, e;
    chunk_range(n, groups, blockIdx.x, kBktTile, b, e);
    uint32_t key[kBktItems];
    auto load = [&](uint64_t i0, uint32_t (&kk)[kBktItems]) {
#pragma unroll
        for (int k = 0; k < kBktItems; k++) {
            const uint64_t i = i0 + (uint64_t)k * kBktThreads + t;
            kk[k] = i < e ? (uint32_t)(in[i] >> 32) : 0xffffffffu;
        }
    };
    load(b, key);   // the first tile's keys travel together with the splitters: one memory round trip
    bkt_load_splitters<B>(s_S, splitters);
    for (uint32_t j = t; j < (uint32_t)B; j += kBktThreads) s_h[j] = 0;
    __syncthreads();
    uint32_t dead = 0;   // culled items all share the last bucket: counted by ballots, not 64-way atomics
    for (uint64_t i0 = b; i0 < e; i0 += kBktTile) {
        // the next tile's keys are in flight while this tile walks the tree (scenes above
        // 1M items give a workgroup several tiles)
        uint32_t nkey[kBktItems];
        if (i0 + kBktTile < e) load(i0 + kBktTile, nkey);
        uint32_t bk[kBktItems];
        bkt_of_n<B>(s_S, key, bk);
#pragma unroll
        for (int k = 0; k < kBktItems; k++) {
            const uint64_t i = i0 + (uint64_t)k * kBktThreads + t;
            const bool d = key[k] == 0xffffffffu;
            dead += (uint32_t)__popcll(__ballot(d && i < e));
            if (!d) atomicAdd(&s_h[bk[k]], 1u);
            if (bid && i < e) bid[i] = (uint16_t)bk[k];   // the scatter reads it instead of searching again
        }
        if (i0 + kBktTile < e) {
#pragma unroll
            for (int k = 0; k < kBktItems; k++) key[k] = nkey[k];
        }
    }
    if (lane == 0 && dead) atomicAdd(&s_h[B - 1], dead);
    __syncthreads();
    // chunk-major (hist[chunk][bucket]): this workgroup's row is one coalesced 4B-per-bucket run
    // (bucket-major, each of its B words went to another cache line: 15 us for 1M items)
    for (uint32_t j = t; j < (uint32_t)B; j += kBktThreads) hist[(size_t)blockIdx.x * B + j] = s_h[j];
}

// Per bucket, the exclusive scan over the chunks of the chunk-major histogram (in place)
// and the bucket's total.  64 buckets per workgroup (one per lane), 16 waves splitting the
// chunks: every load is a coalesced 256-B row segment.  groups <= kBktMaxGroups.
constexpr int kBktMaxGroups = kMaxBucketGroups;
template <int B>
__global__ __launch_bounds__(1024) void k_bkt_scan(uint32_t* __restrict__ hist, int groups,
                                                   uint32_t* __restrict__ totals) {
    GSR_GEOM_PRIO();
    constexpr int kPerMax = kBktMaxGroups / 16;
    __shared__ uint32_t s_part[16][64];
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    const uint32_t b = blockIdx.x * 64u + lane;
    const uint32_t per = ((uint32_t)groups + 15u) / 16u;
    const uint32_t g0 = w * per;
    uint32_t v[kPerMax], sum = 0;
#pragma unroll
    for (int i = 0; i < kPerMax; i++) {
        const uint32_t g = g0 + (uint32_t)i;
        v[i] = (uint32_t)i < per && g < (uint32_t)groups ? hist[(size_t)g * B + b] : 0u;
        sum += v[i];
    }
    s_part[w][lane] = sum;
    __syncthreads();
    uint32_t run = 0, tot = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) {
        const uint32_t p = s_part[k][lane];
        run += k < w ? p : 0u;
        tot += p;
    }
    if (w == 0) totals[b] = tot;
    // the frame's "a live item has key 0xFFFFFFFF" word (bkt_sat_word), raised by the scatter
    if (blockIdx.x == 0 && t == 0) totals[2 * B + 1] = 0u;
#pragma unroll
    for (int i = 0; i < kPerMax; i++) {
        const uint32_t g = g0 + (uint32_t)i;
        if ((uint32_t)i < per && g < (uint32_t)groups) {
            hist[(size_t)g * B + b] = run;
            run += v[i];
        }
    }
}

// The big buckets' scan (kBigBuckets buckets, up to kBigBucketGroups chunks: k_bkt_scan's
// layout put 1.25 MB through 8 workgroups, 23 us at 611 chunks): 16 buckets per 1,024-thread
// workgroup, each wave's four 16-lane quarters reading a 64-B row segment of four different
// chunks (64 chunk slices per workgroup), the slices' sums combined in LDS.  B / 16
// workgroups.  (A wave per bucket measured 8.5 against 5.9 us)
__global__ __launch_bounds__(1024) void k_bkt_scan_g(uint32_t* __restrict__ hist, int groups,
                                                     uint32_t* __restrict__ totals) {
    GSR_GEOM_PRIO();
    constexpr int B = kBigBuckets;
    constexpr int kPerMax = (kBigBucketGroups + 63) / 64;
    __shared__ uint32_t s_part[64][16];
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    const uint32_t bl = lane & 15u, sl = w * 4u + (lane >> 4);   // bucket in the group, chunk slice
    const uint32_t b = blockIdx.x * 16u + bl;
    const uint32_t per = ((uint32_t)groups + 63u) / 64u;
    const uint32_t g0 = sl * per;
    uint32_t v[kPerMax], sum = 0;
#pragma unroll
    for (int i = 0; i < kPerMax; i++) {
        const uint32_t g = g0 + (uint32_t)i;
        v[i] = (uint32_t)i < per && g < (uint32_t)groups ? hist[(size_t)g * B + b] : 0u;
        sum += v[i];
    }
    s_part[sl][bl] = sum;
    __syncthreads();
    uint32_t run = 0, tot = 0;
    for (uint32_t k = 0; k < 64u; k++) {
        const uint32_t p = s_part[k][bl];
        run += k < sl ? p : 0u;
        tot += p;
    }
    if (sl == 0) totals[b] = tot;
    if (blockIdx.x == 0 && t == 0) totals[2 * B + 1] = 0u;   // bkt_sat_word (as k_bkt_scan)
#pragma unroll
    for (int i = 0; i < kPerMax; i++) {
        const uint32_t g = g0 + (uint32_t)i;
        if ((uint32_t)i < per && g < (uint32_t)groups) {
            hist[(size_t)g * B + b] = run;
            run += v[i];
        }
    }
}

// 16-bit half h of the packed counter word v.
__device__ __forceinline__ uint32_t half16(uint32_t v, uint32_t h) { return (v >> (16u * h)) & 0xffffu; }

// Bucket records: 16 B {index, key, rect, 0} (R12 false: one store request per item in the
// unstaged scatter), or 12 B {index, key, rect} (R12: the staged scatter writes runs, where
// the bytes, not the requests, bound it; a quarter fewer of them).
struct __attribute__((packed, aligned(4))) BktRec12 {
    uint32_t i, k, r;
};
template <bool R12>
__device__ __forceinline__ uint4 rec_get(const uint4* __restrict__ rec, uint32_t q) {
    if (R12) {
        const BktRec12 v = reinterpret_cast<const BktRec12*>(rec)[q];
        return make_uint4(v.i, v.k, v.r, 0u);
    }
    return rec[q];
}
template <bool R12>
__device__ __forceinline__ void rec_put(uint4* __restrict__ rec, uint32_t q, uint32_t i, uint32_t k, uint32_t r) {
    if (R12) reinterpret_cast<BktRec12*>(rec)[q] = BktRec12{i, k, r};
    else rec[q] = make_uint4(i, k, r, 0u);
}

// bstart (B + 2 words): written by chunk 0's workgroup, the first position of every bucket
// and bstart[B] = n (k_bkt_local reads its bucket's range there); bstart[B + 1] (cleared by
// k_bkt_scan) is raised when a live item (a tile rect that covers tiles) has key 0xFFFFFFFF.
// TH threads (512 from 512 buckets up: twice the waves of 256, half the items per wave, so
// each wave's latency chain is half as long; the grid is only ~n / 2,048 workgroups:
// 16.3-16.8 -> 15.6-15.8 us at config 2, profiles/r05_kt_bkt_scatter512.txt).
// Live items go out as one 16-B record {index, key, rect, 0} into rec (one store request per
// item: a 4,096-way scatter writes ~one item per bucket per tile, so every store of a wave hits
// its own cache line and the scatter is bound by the L2's request rate, not by bytes: two
// arrays, item and rect, were two requests per item); k_bkt_local reads a bucket's records
// back contiguously.  The last bucket (key 0xFFFFFFFF, never sorted) goes straight to its
// final place in out / pay_out.  The next tile's items and rects are loaded while this one
// is ranked.
// STAGED (the big buckets' scatter): the tile is laid out in LDS by bucket first (tile-local
// position = the bucket's offset in the tile + the item's stable rank in it), then written out
// by position, so the lanes of a store that hold items of one bucket write consecutive 12-B
// records (a run per bucket and tile: ~4 items at 512 buckets) instead of one store request
// each.  It takes every item's bucket from the count kernel (bid) instead of searching the
// splitters again, and thread t < B / 2 owns counter word t (buckets 2t, 2t + 1), so the
// word's wave prefix and the tile offsets' scan are one step; the counters are cleared for the
// next tile after their last read (the stage writes), so a tile starts without a clear +
// barrier: five barriers per tile.  Unstaged (the small kind): the scatter searches the
// splitters itself and writes one 16-B record per item straight from registers.
template <int B, bool RA, int TH, bool STAGED>
__global__ __launch_bounds__(TH) __attribute__((amdgpu_waves_per_eu(1))) void k_bkt_scatter(const uint64_t* __restrict__ in,
                                                             uint64_t* __restrict__ out, uint32_t n,
                                                             const uint32_t* __restrict__ splitters, int groups,
                                                             const uint32_t* __restrict__ hist,
                                                             const uint32_t* __restrict__ totals,
                                                             const uint32_t* __restrict__ rect,
                                                             uint32_t* __restrict__ pay_out,
                                                             uint32_t* __restrict__ bstart,
                                                             uint4* __restrict__ rec,
                                                             const uint16_t* __restrict__ bid) {
    GSR_GEOM_PRIO();
    constexpr uint32_t TILE = kBktTile;
    constexpr int NW = TH / 64, kIt = TILE / TH;  // waves; items per thread
    constexpr uint32_t kW = B / 2;                      // packed counter words per wave
    constexpr int kPer = B / TH;                        // buckets per thread (scan)
    constexpr int kWPer = (kW + TH - 1) / TH;           // counter words per thread
    static_assert(kPer >= 1 && kIt * TH == TILE, "bucket / thread split");
    static_assert(!STAGED || B / 2 <= TH, "staged: one counter word per thread");
    __shared__ uint32_t s_S[B], s_gbase[B];
    __shared__ uint32_t s_wc[NW][kW];
    __shared__ uint32_t s_scr[NW];
    // STAGED: per-bucket tile offsets, the tile in bucket order
    __shared__ uint32_t s_tp[STAGED ? B : 1];
    __shared__ uint4 s_stage[STAGED ? TILE : 1];
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    const uint64_t lt_mask = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    const int chunk = xcd_chunk((int)blockIdx.x, groups);   // each XCD takes a contiguous run of chunks
    uint64_t b, e;
    chunk_range(n, groups, chunk, kBktTile, b, e);   // chunks as k_bkt_count's
    const uint32_t wbase = w * 64 * kIt;
    uint64_t it[kIt];
    uint32_t pv[kIt], bv[kIt];
    // STAGED: the count kernel's bucket of every item (bid), loaded with the tile
    auto load = [&](uint64_t tb, uint32_t tn, uint64_t (&ii)[kIt], uint32_t (&pp)[kIt], uint32_t (&bb)[kIt]) {
#pragma unroll
        for (int k = 0; k < kIt; k++) {
            const uint32_t el = wbase + k * 64 + lane;
            ii[k] = el < tn ? in[tb + el] : ~0ull;
            pp[k] = el < tn ? rect[tb + el] : 0u;   // the input is the preprocess order: rect by position
            if (STAGED) bb[k] = el < tn ? (uint32_t)bid[tb + el] : (uint32_t)B - 1u;
        }
    };
    // the first tile's items and rects, the splitters, the bucket totals and this chunk's
    // histogram row are all loaded in one memory round trip
    load(b, (uint32_t)min((uint64_t)TILE, e - b), it, pv, bv);
    if (!STAGED) bkt_load_splitters<B, TH>(s_S, splitters);
    {   // this chunk's first slot in every bucket: the bucket's start + the earlier chunks' items
        uint32_t loc[kPer], hrow[kPer], sum = 0;
#pragma unroll
        for (int k = 0; k < kPer; k++) {
            loc[k] = totals[t * kPer + k];
            hrow[k] = hist[(size_t)chunk * B + t * kPer + k];
            sum += loc[k];
        }
        uint32_t tot;
        uint32_t run = block_exclusive_scan<uint32_t, NW>(sum, s_scr, tot);
#pragma unroll
        for (int k = 0; k < kPer; k++) {
            const uint32_t d = t * kPer + k;
            if (chunk == 0) bstart[d] = run;
            s_gbase[d] = run + hrow[k];
            run += loc[k];
        }
        if (chunk == 0 && t == 0) bstart[B] = n;
    }
    if (b >= e) return;   // uniform per workgroup, after the scan's barriers
    if (STAGED) {   // the first tile's counter clear; every later one follows the stage writes
        for (uint32_t j = t; j < NW * kW; j += TH) (&s_wc[0][0])[j] = 0;
        __syncthreads();
    }
    for (uint64_t tb = b; tb < e; tb += TILE) {
        const uint32_t tn = (uint32_t)min((uint64_t)TILE, e - tb);
        const bool more = tb + TILE < e;   // uniform
        uint64_t nit[kIt];
        uint32_t npv[kIt], nbv[kIt];
        if (more) load(tb + TILE, (uint32_t)min((uint64_t)TILE, e - tb - TILE), nit, npv, nbv);
        if (!STAGED) {
            for (uint32_t j = t; j < NW * kW; j += TH) (&s_wc[0][0])[j] = 0;
            __syncthreads();
        }
        uint32_t dg[kIt], rk[kIt], keys[kIt];
#pragma unroll
        for (int k = 0; k < kIt; k++) keys[k] = (uint32_t)(it[k] >> 32);
        if (STAGED) {
#pragma unroll
            for (int k = 0; k < kIt; k++) dg[k] = bv[k];
        } else {
            bkt_of_n<B>(s_S, keys, dg);   // a key 0xFFFFFFFF (culled) counts every splitter: bucket B - 1
        }
        // culled items (the last bucket) rank by ballot against a running wave count, so the
        // live items' returning atomics have no LDS read between them and stay in flight together
        uint32_t dead_run = 0;
        uint32_t old[kIt];
#pragma unroll
        for (int k = 0; k < kIt; k++) {
            const uint32_t el = wbase + k * 64 + lane;
            const bool valid = el < tn;
            const bool dead = keys[k] == 0xffffffffu;
            const uint32_t d = dg[k];
            // a live Gaussian whose key saturated (depth >= ~4295 under a far clip that keeps
            // it) shares the last bucket with the culled items: k_bkt_local's fused row count
            // must then bin that bucket too (rare: a plain vector store of 1)
            if (valid && dead && rect_count(unpack_rect(pv[k]))) bstart[B + 1] = 1u;
            const uint64_t dm = __ballot(valid && dead);
            uint32_t r = dead_run + (uint32_t)__popcll(dm & lt_mask);
            dead_run += (uint32_t)__popcll(dm);
            const uint32_t sh = 16u * (d & 1u);
            if (RA) {
                // every lane adds (0 when it has no live item): no branch, so the eight returning
                // atomics are in flight together; the halves are taken after the loop
                old[k] = atomicAdd(&s_wc[w][d >> 1], valid && !dead ? 1u << sh : 0u);
            } else {
                const uint64_t peers = match_peers<12>(d, valid && !dead, 12);   // every lane takes part
                if (valid && !dead) {
                    r = half16(s_wc[w][d >> 1], d & 1u) + (uint32_t)__popcll(peers & lt_mask);
                    if (lane == (uint32_t)(__ffsll((unsigned long long)peers) - 1))
                        atomicAdd(&s_wc[w][d >> 1], (uint32_t)__popcll(peers) << sh);
                }
            }
            rk[k] = r;
        }
        if (RA) {
#pragma unroll
            for (int k = 0; k < kIt; k++)
                if (keys[k] != 0xffffffffu) rk[k] = half16(old[k], dg[k] & 1u);
        }
        if (lane == 0 && dead_run) atomicAdd(&s_wc[w][(B - 1) >> 1], dead_run << 16);   // B - 1 is odd: high half
        __syncthreads();
        // per word (two buckets): exclusive prefix over the waves in place, tile counts kept
        // (halves <= TILE <= 32,768: no carry between them)
        uint32_t tc[kWPer];
#pragma unroll
        for (int q = 0; q < kWPer; q++) {
            const uint32_t j = t + q * TH;
            tc[q] = 0;
            if (j < kW) {
                uint32_t c[NW];
#pragma unroll
                for (int v = 0; v < NW; v++) c[v] = s_wc[v][j];
                uint32_t run = 0;
#pragma unroll
                for (int v = 0; v < NW; v++) {
                    s_wc[v][j] = run;
                    run += c[v];
                }
                tc[q] = run;
            }
        }
        if (STAGED) {
            // the buckets' offsets in the tile: thread t < kW scans word t's two tile counts
            const uint32_t lo = tc[0] & 0xffffu, hi = tc[0] >> 16;
            uint32_t tot;
            const uint32_t ex = block_exclusive_scan_lead<uint32_t, NW>(t < kW ? lo + hi : 0u, s_scr, tot);
            if (t < kW) {
                s_tp[2 * t] = ex;
                s_tp[2 * t + 1] = ex + lo;
            }
        }
        __syncthreads();
        if (STAGED) {
#pragma unroll
            for (int k = 0; k < kIt; k++) {
                const uint32_t el = wbase + k * 64 + lane;
                if (el < tn) {
                    const uint32_t d = dg[k];
                    const uint32_t p = s_tp[d] + half16(s_wc[w][d >> 1], d & 1u) + rk[k];
                    s_stage[p] = make_uint4((uint32_t)it[k], (uint32_t)(it[k] >> 32), pv[k], d);
                }
            }
            __syncthreads();
            // the counters' last read is behind: clear them for the next tile
            for (uint32_t j = t; j < NW * kW; j += TH) (&s_wc[0][0])[j] = 0;
            for (uint32_t q = t; q < tn; q += TH) {
                const uint4 r = s_stage[q];
                const uint32_t d = r.w;
                const uint32_t dst = s_gbase[d] + (q - s_tp[d]);
                if (d == (uint32_t)B - 1u) {
                    out[dst] = ((uint64_t)r.y << 32) | r.x;
                    pay_out[dst] = r.z;
                } else {
                    rec_put<true>(rec, dst, r.x, r.y, r.z);
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < kIt; k++) {
                const uint32_t el = wbase + k * 64 + lane;
                if (el < tn) {
                    const uint32_t d = dg[k];
                    const uint32_t dst = s_gbase[d] + half16(s_wc[w][d >> 1], d & 1u) + rk[k];
                    if (d == (uint32_t)B - 1u) {
                        out[dst] = it[k];
                        pay_out[dst] = pv[k];
                    } else {
                        rec_put<false>(rec, dst, (uint32_t)it[k], (uint32_t)(it[k] >> 32), pv[k]);
                    }
                }
            }
        }
        if (more) {
#pragma unroll
            for (int k = 0; k < kIt; k++) {
                it[k] = nit[k];
                pv[k] = npv[k];
                if (STAGED) bv[k] = nbv[k];
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kWPer; q++) {
            const uint32_t j = t + q * TH;
            if (j < kW) {
                s_gbase[2 * j] += tc[q] & 0xffffu;
                s_gbase[2 * j + 1] += tc[q] >> 16;
            }
        }
        // the next tile's barrier after the ranking atomics (STAGED), or its counter clear and
        // barrier (unstaged), orders these updates before their use
    }
}

// Next frame's splitters from this bucket's part of the sorted live order: splitter j is
// the key at live position floor((j + 1) * live / (B - 1)), j < B - 2.  key_at(q) reads
// the sorted key at bucket-local position q.
// Where splitter j (j < B - 2) is taken in a sorted live order of `live` items: the open
// first and last live buckets get a quarter of an interior bucket's share, so a moving
// camera's drift past the previous frame's nearest and farthest keys (which lands in
// them) has room under the local capacity (config 2 on a 0.25-deg orbit, the first frames
// after the LSD quantiles: the last bucket held 2,058 items, over the 2,048 capacity, at
// an even split).  pos(j) = floor(N(j) live / D), N(j) = (B - 3) + j (4B - 6),
// D = 4 (B - 3)(B - 1): pos(0) = live / (4 (B - 1)), pos(B - 3) = live (1 - 1 / (4 (B - 1))).
template <int B>
__device__ __forceinline__ uint32_t bkt_split_pos(uint32_t j, uint32_t live) {
    constexpr uint64_t D = 4ull * (uint64_t)(B - 3) * (uint64_t)(B - 1);
    return (uint32_t)(((uint64_t)(B - 3) + (uint64_t)j * (uint64_t)(4 * B - 6)) * live / D);
}
// The smallest j with bkt_split_pos(j, live) >= s (live > 0).
template <int B>
__device__ __forceinline__ uint64_t bkt_split_first(uint64_t s, uint32_t live) {
    constexpr uint64_t D = 4ull * (uint64_t)(B - 3) * (uint64_t)(B - 1);
    const uint64_t c = (s * D + live - 1) / live;   // pos(j) >= s  <=>  N(j) >= c
    return c <= (uint64_t)(B - 3) ? 0ull : (c - (uint64_t)(B - 3) + (uint64_t)(4 * B - 7)) / (uint64_t)(4 * B - 6);
}

template <int B, int TH = kBktThreads, typename KeyAt>
__device__ __forceinline__ void bkt_write_splitters(uint32_t start, uint32_t count, uint32_t live,
                                                    uint32_t* __restrict__ s_out, KeyAt key_at) {
    if (live == 0 || count == 0) return;
    // splitters j in [j0, j1) are taken at positions in [start, start + count)
    const uint64_t j0 = bkt_split_first<B>(start, live);
    const uint64_t j1 = min(bkt_split_first<B>((uint64_t)start + count, live), (uint64_t)B - 2u);
    for (uint64_t j = j0 + threadIdx.x; j < j1; j += TH)
        s_out[j] = key_at(bkt_split_pos<B>((uint32_t)j, live) - start);
}

// Row-pass histograms of one chunk of the depth order (k_bin_rows_count's, for the chunk
// of the bucket this workgroup sorted): per tile row the row items and the pairs of its
// rects, as difference arrays in LDS (per wave), then a prefix over the rows.
// hist[row][g] and hist[256 + row][g], rows < tiles_y.
struct RowHist {
    uint32_t* hist;      // nullptr: not fused (the row pass counts for itself)
    int groups;          // the row pass's chunks: the live buckets (B - 1)
    int tiles_y;
};

__device__ __forceinline__ void row_hist_add(uint32_t (*h_items)[256], uint32_t (*h_pairs)[256], uint32_t w,
                                             uint32_t packed) {
    const uint64_t r = unpack_rect(packed);
    if (rect_count(r)) {
        const uint32_t ty0 = (uint32_t)((r >> 32) & 0xffffu), ty1 = (uint32_t)(r >> 48);
        const uint32_t cols = rect_cols(r);
        atomicAdd(&h_items[w][ty0], 1u);
        atomicAdd(&h_pairs[w][ty0], cols);
        if (ty1 < 255u) {
            atomicSub(&h_items[w][ty1 + 1], 1u);
            atomicSub(&h_pairs[w][ty1 + 1], cols);
        }
    }
}

__device__ __forceinline__ void row_hist_write(const RowHist& rh, uint32_t g, uint32_t (*h_items)[256],
                                               uint32_t (*h_pairs)[256], uint32_t* s_scr) {
    const uint32_t t = threadIdx.x;
    __syncthreads();
    const uint32_t di = h_items[0][t] + h_items[1][t] + h_items[2][t] + h_items[3][t];
    const uint32_t dp = h_pairs[0][t] + h_pairs[1][t] + h_pairs[2][t] + h_pairs[3][t];
    uint32_t ti, tp;
    const uint32_t ci = block_exclusive_scan<uint32_t>(di, s_scr, ti) + di;
    const uint32_t cp = block_exclusive_scan<uint32_t>(dp, s_scr, tp) + dp;
    if (t < (uint32_t)rh.tiles_y) {
        rh.hist[t * (uint32_t)rh.groups + g] = ci;
        rh.hist[(256 + t) * (uint32_t)rh.groups + g] = cp;
    }
}

// One workgroup per live bucket (grid B - 1; B with the fused row count, whose last
// workgroup only counts the last bucket's rows).  bstart: the buckets' first positions
// (k_bkt_scatter); s_in: the splitters this frame was bucketed by, which bound the keys of
// every bucket but the first and the last (their key span sets the passes).  cap: buckets
// above it take the global path (kBktCap; smaller only as a test hook).  over_host
// (host-mapped, nullable): items sorted by the global path, for the diagnostics.
template <int B, bool RA, bool R12 = false>
__global__ __launch_bounds__(kBktThreads) void k_bkt_local(uint64_t* __restrict__ items, uint64_t* __restrict__ scratch,
                                                           uint32_t* __restrict__ pay, uint32_t* __restrict__ pay_scratch,
                                                           uint32_t* __restrict__ bstart,
                                                           const uint32_t* __restrict__ s_in,
                                                           uint32_t* __restrict__ s_next, uint32_t cap,
                                                           unsigned int* over_host, RowHist rh,
                                                           const uint4* __restrict__ rec,
                                                           const uint32_t* __restrict__ only = nullptr) {
    GSR_GEOM_PRIO();
    __shared__ uint64_t s_items[kBktTile];
    __shared__ uint32_t s_pay[kBktTile];
    __shared__ uint32_t s_wc[4][256], s_lbase[256], s_gb[256];
    __shared__ uint32_t s_hp[4][256];   // fused row-pass count: pairs (s_wc holds the items)
    __shared__ uint32_t s_scr[4], s_mm[2];
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    auto row_zero = [&]() {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            s_wc[k][t] = 0;
            s_hp[k][t] = 0;
        }
    };
    if (blockIdx.x == (uint32_t)B - 1u) {
        // fused row count only (grid B): the last bucket (key 0xFFFFFFFF, index order, never
        // sorted) is the row pass's last chunk.  It holds culled items only unless the scatter
        // raised bstart[B + 1]; then its rects are counted (every live one binned, as the LSD
        // path and render.cu do), else the chunk is emptied (bstart[B] = its start: the
        // row pass reads nothing there).  Only this workgroup reads bstart[B].
        const uint32_t start = bstart[B - 1], end = bstart[B];
        const bool sat = bstart[B + 1] != 0u;
        row_zero();
        __syncthreads();
        if (sat) {
            for (uint32_t i = start + t; i < end; i += 4u * kBktThreads) {
                uint32_t p[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const uint32_t j = i + (uint32_t)k * kBktThreads;
                    p[k] = j < end ? pay[j] : pack_rect(kDeadRect);
                }
#pragma unroll
                for (int k = 0; k < 4; k++) row_hist_add(s_wc, s_hp, w, p[k]);
            }
        }
        row_hist_write(rh, (uint32_t)B - 1u, s_wc, s_hp, s_scr);
        if (!sat && t == 0) bstart[B] = start;
        return;
    }
    // XCD-contiguous buckets: the fused row count's histogram lines (16 consecutive
    // buckets of a row) merge in one L2 (12.4 -> 11.95 us at config 2,
    // profiles/r05_kt_xcd_hist.txt)
    const uint32_t bkt = (uint32_t)xcd_chunk((int)blockIdx.x, B - 1);
    if (only && only[bkt] == 0u) return;   // big buckets: only those k_bbk_local left to this kernel
    const uint32_t start = bstart[bkt], count = bstart[bkt + 1] - start, live = bstart[B - 1];
    // keys of bucket b lie in [s_in[b - 1], s_in[b]) for 0 < b < B - 2
    const bool bounded = bkt > 0 && bkt < (uint32_t)B - 2u;
    const uint32_t klo = bounded ? s_in[bkt - 1] : 0u, khi = bounded ? s_in[bkt] : 0u;
    if (bkt == 0 && t == 0) {
        s_next[B - 2] = 0xffffffffu;
        if (live == 0)   // no live quantiles (a camera looking away): keep this frame's splitters
            for (uint32_t j = 0; j < (uint32_t)B - 2u; j++) s_next[j] = s_in[j];
    }
    if (count == 0) {   // uniform; an empty bucket is an empty row-pass chunk
        if (rh.hist) {
            row_zero();
            row_hist_write(rh, bkt, s_wc, s_hp, s_scr);
        }
        return;
    }
    uint64_t* const seg = items + start;
    uint32_t* const pseg = pay + start;
    auto rseg = [&](uint32_t q) { return rec_get<R12>(rec, start + q); };   // the bucket's records, index order
    // ---- fast path: the bucket in registers, stable 8-bit passes through LDS.  IT items per
    // thread: 4 for buckets of up to 1,024 (the usual ~n / B: every wave holds a quarter of
    // the bucket), 8 up to the capacity (at 8, buckets under 1,024 left waves 2 and 3 idle
    // and waves 0 and 1 with twice the slots) ----
    auto fast = [&](auto it_c) {
        constexpr int IT = decltype(it_c)::value;
        const uint32_t wbase = w * 64 * IT;
        uint64_t it[IT];
        uint32_t pv[IT];
#pragma unroll
        for (int k = 0; k < IT; k++) {
            const uint32_t el = wbase + k * 64 + lane;
            const uint4 r = el < count ? rseg(el) : make_uint4(~0u, ~0u, 0u, 0u);
            it[k] = ((uint64_t)r.y << 32) | r.x;
            pv[k] = r.z;
        }
        uint32_t kmin = klo, span = khi - klo - 1u;   // bounded: keys in [klo, khi)
        if (!bounded) {   // the open-ended first and last buckets: their own min and max
            uint32_t mn = 0xffffffffu, mx = 0;
#pragma unroll
            for (int k = 0; k < IT; k++)
                if (wbase + k * 64 + lane < count) {
                    mn = min(mn, (uint32_t)(it[k] >> 32));
                    mx = max(mx, (uint32_t)(it[k] >> 32));
                }
            mn = ~wave_max_u32(~mn);
            mx = wave_max_u32(mx);
            if (t < 2) s_mm[t] = t ? 0u : 0xffffffffu;
            __syncthreads();
            if (lane == 0) {
                atomicMin(&s_mm[0], mn);
                atomicMax(&s_mm[1], mx);
            }
            __syncthreads();
            kmin = s_mm[0];
            span = s_mm[1] - kmin;
        }
        const int bits = span ? 32 - __clz((int)span) : 0;
        for (int shift = 0; shift < bits; shift += 8) {   // uniform
            uint32_t dig[IT], pos[IT];
#pragma unroll
            for (int k = 0; k < IT; k++) dig[k] = (((uint32_t)(it[k] >> 32) - kmin) >> shift) & 0xffu;
            (void)bin_rank_tile<IT, 8, RA>(dig, count, pos, s_wc, s_lbase, s_scr);
#pragma unroll
            for (int k = 0; k < IT; k++) {
                const uint32_t el = wbase + k * 64 + lane;
                if (el < count) {
                    s_items[pos[k]] = it[k];
                    s_pay[pos[k]] = pv[k];
                }
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < IT; k++) {
                const uint32_t el = wbase + k * 64 + lane;
                if (el < count) {
                    it[k] = s_items[el];
                    pv[k] = s_pay[el];
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int k = 0; k < IT; k++) {
            const uint32_t el = wbase + k * 64 + lane;
            if (el < count) {
                seg[el] = it[k];
                pseg[el] = pv[k];
                s_items[el] = it[k];
            }
        }
        if (rh.hist) {   // the bucket is the row pass's chunk: its row histograms from the rects
            row_zero();
            __syncthreads();
#pragma unroll
            for (int k = 0; k < IT; k++)
                if (wbase + k * 64 + lane < count) row_hist_add(s_wc, s_hp, w, pv[k]);
            row_hist_write(rh, bkt, s_wc, s_hp, s_scr);
        }
        __syncthreads();
        if (bkt < (uint32_t)B - 1u)
            bkt_write_splitters<B>(start, count, live, s_next,
                                   [&](uint32_t q) { return (uint32_t)(s_items[q] >> 32); });
    };
    // (5 and 6 items per thread for the 1,025-1,536-item buckets of scenes above 4M items:
    // at 8 the items of a 1,220-item bucket sat on waves 0-1 and 2-3 idled)
    if (count <= min(cap, (uint32_t)kBktThreads * 4u)) {
        fast(std::integral_constant<int, 4>{});
        return;
    }
    if (count <= min(cap, (uint32_t)kBktThreads * 5u)) {
        fast(std::integral_constant<int, 5>{});
        return;
    }
    if (count <= min(cap, (uint32_t)kBktThreads * 6u)) {
        fast(std::integral_constant<int, 6>{});
        return;
    }
    if (count <= cap) {
        fast(std::integral_constant<int, 8>{});
        return;
    }
    const uint32_t wbase = w * 64 * kBktItems;
    // ---- over capacity: stable 8-bit passes through global memory, one tile at a time ----
    if (over_host && t == 0) atomicAdd_system(over_host, count);
    for (uint32_t i = t; i < count; i += kBktThreads) {   // the records into the item / rect arrays
        const uint4 r = rseg(i);
        seg[i] = ((uint64_t)r.y << 32) | r.x;
        pseg[i] = r.z;
    }
    __threadfence();
    __syncthreads();
    uint32_t kmin = 0xffffffffu, kmax = 0;
    for (uint32_t i = t; i < count; i += kBktThreads) {
        const uint32_t k = (uint32_t)(seg[i] >> 32);
        kmin = min(kmin, k);
        kmax = max(kmax, k);
    }
    kmin = ~wave_max_u32(~kmin);
    kmax = wave_max_u32(kmax);
    if (t < 2) s_mm[t] = t ? 0u : 0xffffffffu;
    __syncthreads();
    if (lane == 0) {
        atomicMin(&s_mm[0], kmin);
        atomicMax(&s_mm[1], kmax);
    }
    __syncthreads();
    kmin = s_mm[0];
    const uint32_t span = s_mm[1] - kmin;
    const int bits = span ? 32 - __clz((int)span) : 0;
    if (over_host && t == 0 && bits) atomicAdd_system(over_host + 1, count * (uint32_t)((bits + 7) / 8));
    uint64_t* src = seg;
    uint64_t* dst = scratch + start;
    uint32_t* psrc = pseg;
    uint32_t* pdst = pay_scratch + start;
    int passes = 0;
    for (int shift = 0; shift < bits; shift += 8, ++passes) {
        auto digit = [&](uint64_t v) { return (((uint32_t)(v >> 32) - kmin) >> shift) & 0xffu; };
        s_gb[t] = 0;
        __syncthreads();
        for (uint32_t i = t; i < count; i += kBktThreads) atomicAdd(&s_gb[digit(src[i])], 1u);
        __syncthreads();
        {
            const uint32_t c = s_gb[t];
            uint32_t tot;
            const uint32_t ex = block_exclusive_scan<uint32_t>(c, s_scr, tot);
            s_gb[t] = ex;   // every read of s_gb[t] (its own count) is done by this thread
        }
        for (uint32_t tb = 0; tb < count; tb += kBktTile) {
            const uint32_t tn = min(kBktTile, count - tb);
            uint64_t it[kBktItems];
            uint32_t pv[kBktItems], dig[kBktItems], pos[kBktItems];
#pragma unroll
            for (int k = 0; k < kBktItems; k++) {
                const uint32_t el = wbase + k * 64 + lane;
                it[k] = el < tn ? src[tb + el] : ~0ull;
                pv[k] = el < tn ? psrc[tb + el] : 0u;
                dig[k] = digit(it[k]);
            }
            const uint32_t tcount = bin_rank_tile<kBktItems, 8, RA>(dig, tn, pos, s_wc, s_lbase, s_scr);
#pragma unroll
            for (int k = 0; k < kBktItems; k++) {
                const uint32_t el = wbase + k * 64 + lane;
                if (el < tn) {
                    s_items[pos[k]] = it[k];
                    s_pay[pos[k]] = pv[k];
                }
            }
            __syncthreads();
            for (uint32_t q = t; q < tn; q += kBktThreads) {
                const uint64_t v = s_items[q];
                const uint32_t d = digit(v);
                const uint32_t o = s_gb[d] + (q - s_lbase[d]);
                dst[o] = v;
                pdst[o] = s_pay[q];
            }
            __syncthreads();
            s_gb[t] += tcount;
            // bin_rank_tile's first barrier orders this before the next tile's reads
        }
        __threadfence();   // the next pass (other waves of this workgroup) reads what this one wrote
        __syncthreads();
        uint64_t* ts = src;
        src = dst;
        dst = ts;
        uint32_t* tp = psrc;
        psrc = pdst;
        pdst = tp;
    }
    if (passes & 1) {   // the result is in the scratch segment: copy it back
        for (uint32_t i = t; i < count; i += kBktThreads) {
            seg[i] = src[i];
            pseg[i] = psrc[i];
        }
        __threadfence();
        __syncthreads();
    }
    if (rh.hist) {
        row_zero();
        __syncthreads();
        for (uint32_t i = t; i < count; i += kBktThreads) row_hist_add(s_wc, s_hp, w, pseg[i]);
        row_hist_write(rh, bkt, s_wc, s_hp, s_scr);
    }
    if (bkt < (uint32_t)B - 1u)
        bkt_write_splitters<B>(start, count, live, s_next, [&](uint32_t q) { return (uint32_t)(seg[q] >> 32); });
}

// ---- big buckets (scenes above 2M Gaussians: 512 buckets of ~n / 512 items) ----
//
// One 1,024-thread workgroup sorts a bucket of up to 16,384 items in LDS: up to 16 per thread
// (blocked per wave, so a wave's items are consecutive positions; the 16 waves share the
// bucket evenly, ceil(count / 1,024) rows of 64 each, so all of them work), stable 8-bit LSD passes
// over key - lo whose exchange carries one u32 per item, slot (original position, 14 bits) |
// (key - lo) << 14, so keys may span 18 bits above lo (config 3's buckets: 12-13).  After
// the last pass each position knows its slot and key; the index (kept in LDS by slot) and
// the rect (pulled through the exchange buffer by slot) join them and the bucket is written
// out coalesced.  Buckets over the capacity or wider than 18 bits are flagged in `left` and
// sorted by k_bkt_local's paths in a second launch.
constexpr int kBbThreads = 1024;
constexpr int kBbItems = 16;                            // capacity kBbThreads * 16: 16,384

// One workgroup per CU; it reads the staged scatter's 12-B records.
template <bool RA>
__global__ __launch_bounds__(kBbThreads) void k_bbk_local(uint64_t* __restrict__ items, uint32_t* __restrict__ pay,
                                                          const uint32_t* __restrict__ bstart,
                                                          const uint32_t* __restrict__ s_in,
                                                          uint32_t* __restrict__ s_next, uint32_t cap,
                                                          const uint4* __restrict__ rec, uint32_t* __restrict__ left) {
    GSR_GEOM_PRIO();
    constexpr int B = kBigBuckets, TH = kBbThreads;
    constexpr int NW = TH / 64;
    constexpr uint32_t kCap = (uint32_t)TH * kBbItems;
    constexpr int kBbSlot = __builtin_ctz(kCap);        // slot bits of the exchange word
    constexpr int kBbKeyBits = 32 - kBbSlot;            // key bits above lo it carries
    __shared__ uint32_t s_buf[kCap];                    // the exchange, then the rect pull, then the keys
    __shared__ uint32_t s_idx[kCap];                    // the indices by slot
    __shared__ uint32_t s_wc[NW][256];                  // per-wave digit counts, then their wave prefixes
    __shared__ uint32_t s_db[256];                      // the digits' first positions
    __shared__ uint32_t s_scr[NW], s_mm[2];
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    const uint32_t bkt = blockIdx.x;
    const uint32_t start = bstart[bkt], count = bstart[bkt + 1] - start, live = bstart[B - 1];
    const bool bounded = bkt > 0 && bkt < (uint32_t)B - 2u;
    const uint32_t klo = bounded ? s_in[bkt - 1] : 0u, khi = bounded ? s_in[bkt] : 0u;
    if (bkt == 0 && t == 0) {
        s_next[B - 2] = 0xffffffffu;
        if (live == 0)   // no live quantiles (a camera looking away): keep this frame's splitters
            for (uint32_t j = 0; j < (uint32_t)B - 2u; j++) s_next[j] = s_in[j];
    }
    if (count == 0) {
        if (t == 0) left[bkt] = 0u;
        return;
    }
    if (count > min(cap, kCap)) {
        if (t == 0) left[bkt] = 1u;
        return;
    }
    // the waves split the bucket evenly (kk rows of 64 each) so every wave has work
    const uint32_t kk = (count + NW * 64u - 1u) / (NW * 64u), wbase = w * kk * 64u;
    uint32_t x[kBbItems], rct[kBbItems];
    {
        uint32_t key[kBbItems];
#pragma unroll
        for (int k = 0; k < kBbItems; k++) {
            const uint32_t el = wbase + k * 64 + lane;
            const bool in = k < (int)kk && el < count;
            const uint4 r = in ? rec_get<true>(rec, start + el) : make_uint4(0u, 0xffffffffu, 0u, 0u);
            if (in) s_idx[el] = r.x;
            key[k] = r.y;
            rct[k] = r.z;
        }
        uint32_t kmin = klo, span = khi - klo - 1u;
        if (!bounded) {   // the open first and last buckets: their own min and max
            uint32_t mn = 0xffffffffu, mx = 0;
#pragma unroll
            for (int k = 0; k < kBbItems; k++)
                if (k < (int)kk && wbase + k * 64 + lane < count) {
                    mn = min(mn, key[k]);
                    mx = max(mx, key[k]);
                }
            mn = ~wave_max_u32(~mn);
            mx = wave_max_u32(mx);
            if (t < 2) s_mm[t] = t ? 0u : 0xffffffffu;
            __syncthreads();
            if (lane == 0) {
                atomicMin(&s_mm[0], mn);
                atomicMax(&s_mm[1], mx);
            }
            __syncthreads();
            kmin = s_mm[0];
            span = s_mm[1] - kmin;
        }
        if (span >> kBbKeyBits) {   // uniform: wider than the exchange word (k_bkt_local sorts it)
            if (t == 0) left[bkt] = 1u;
            return;
        }
        // the exchange word of every position (before the first pass: position = slot)
#pragma unroll
        for (int k = 0; k < kBbItems; k++) x[k] = (wbase + k * 64 + lane) | ((key[k] - kmin) << kBbSlot);
        __syncthreads();   // every thread has read s_mm before it is rewritten
        if (t == 0) {
            left[bkt] = 0u;
            s_mm[0] = kmin;
            s_mm[1] = span;
        }
    }
    __syncthreads();
    const uint32_t kmin = s_mm[0], span = s_mm[1];
    const int bits = span ? 32 - __clz((int)span) : 0;   // the passes: the bits the keys span
    for (int shift = 0; shift < bits; shift += 8) {   // uniform
        auto digit = [&](int k) { return (x[k] >> (kBbSlot + shift)) & 0xffu; };
        for (uint32_t j = t; j < (uint32_t)NW * 256u; j += TH) (&s_wc[0][0])[j] = 0;
        __syncthreads();
        uint32_t rk[kBbItems];
#pragma unroll
        for (int k = 0; k < kBbItems; k++) {
            rk[k] = 0;
            if (k >= (int)kk) continue;   // uniform
            const uint32_t el = wbase + k * 64 + lane;
            const bool valid = el < count;
            const uint32_t dk = digit(k);
            if (RA) {
                rk[k] = atomicAdd(&s_wc[w][dk], valid ? 1u : 0u);
            } else {
                const uint64_t peers = match_peers<8>(dk, valid, 8);
                rk[k] = 0;
                if (valid) {
                    rk[k] = s_wc[w][dk] + (uint32_t)__popcll(peers & (lane ? (~0ull >> (64 - lane)) : 0ull));
                    if (lane == (uint32_t)(__ffsll((unsigned long long)peers) - 1))
                        atomicAdd(&s_wc[w][dk], (uint32_t)__popcll(peers));
                }
            }
        }
        __syncthreads();
        uint32_t dtot = 0;
        if (t < 256u) {
            uint32_t run = 0;
#pragma unroll
            for (int v = 0; v < NW; v++) {
                const uint32_t c = s_wc[v][t];
                s_wc[v][t] = run;
                run += c;
            }
            dtot = run;
        }
        {
            uint32_t tot;
            const uint32_t ex = block_exclusive_scan<uint32_t, NW>(dtot, s_scr, tot);
            if (t < 256u) s_db[t] = ex;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kBbItems; k++) {
            const uint32_t el = wbase + k * 64 + lane;
            if (k < (int)kk && el < count) {
                const uint32_t dk = digit(k);
                s_buf[s_db[dk] + s_wc[w][dk] + rk[k]] = x[k];
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kBbItems; k++) {
            const uint32_t el = wbase + k * 64 + lane;
            if (k < (int)kk && el < count) x[k] = s_buf[el];
        }
        __syncthreads();
    }
    // rect by slot through the buffer (owners write by slot, positions read), then write out
#pragma unroll
    for (int k = 0; k < kBbItems; k++)
        if (k < (int)kk && wbase + k * 64 + lane < count) s_buf[wbase + k * 64 + lane] = rct[k];
    __syncthreads();
    uint64_t* const seg = items + start;
    uint32_t* const pseg = pay + start;
#pragma unroll
    for (int k = 0; k < kBbItems; k++) {
        const uint32_t el = wbase + k * 64 + lane;
        if (k < (int)kk && el < count) {
            const uint32_t slot = x[k] & (kCap - 1u);
            rct[k] = s_buf[slot];
            seg[el] = ((uint64_t)(kmin + (x[k] >> kBbSlot)) << 32) | s_idx[slot];
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kBbItems; k++) {
        const uint32_t el = wbase + k * 64 + lane;
        if (k < (int)kk && el < count) {
            pseg[el] = rct[k];
            s_buf[el] = kmin + (x[k] >> kBbSlot);   // sorted keys, for the next frame's splitters
        }
    }
    __syncthreads();
    if (bkt < (uint32_t)B - 1u)
        bkt_write_splitters<B, TH>(start, count, live, s_next, [&](uint32_t q) { return s_buf[q]; });
}

// Splitters from a depth order the LSD passes sorted (a context's first frame, or the
// first after the bucket count changed): one workgroup.  live (nullable): the visible
// count of a partitioned sort; else the first key 0xFFFFFFFF is found by two rounds of
// 256 probes and a last scan.
template <int B>
__global__ __launch_bounds__(kBktThreads) void k_bkt_splitters(const uint64_t* __restrict__ items0,
                                                               const uint64_t* __restrict__ items1,
                                                               const uint32_t* __restrict__ dstats, uint32_t n,
                                                               const uint32_t* __restrict__ live_dev,
                                                               uint32_t* __restrict__ s_out) {
    GSR_GEOM_PRIO();
    __shared__ uint32_t s_lo, s_hi;
    const uint64_t* sorted = depth_sorted(items0, items1, dstats);
    const uint32_t t = threadIdx.x;
    uint32_t live;
    if (live_dev) {
        live = min(*live_dev, n);
    } else {
        // the first position whose key is 0xFFFFFFFF (n if none): narrow [lo, hi) by probes
        if (t == 0) {
            s_lo = 0;
            s_hi = n;
        }
        __syncthreads();
        for (int round = 0; round < 3; round++) {
            const uint32_t lo = s_lo, hi = s_hi;
            __syncthreads();
            const uint32_t len = hi - lo;
            if (len <= 1) break;   // uniform
            const uint32_t step = (len + kBktThreads - 1) / kBktThreads;
            const uint32_t p = lo + t * step;
            const bool dead = p < hi && (uint32_t)(sorted[p] >> 32) == 0xffffffffu;
            // the last probe that is live, then the first that is dead, bound the answer
            if (p < hi && !dead) atomicMax(&s_lo, p + 1);
            if (dead) atomicMin(&s_hi, p);
            __syncthreads();
        }
        uint32_t lo = s_lo;
        const uint32_t hi = s_hi;
        __syncthreads();
        // at most a few positions left: each thread checks one
        if (t == 0) s_lo = hi;
        __syncthreads();
        for (uint32_t p = lo + t; p < hi; p += kBktThreads)
            if ((uint32_t)(sorted[p] >> 32) == 0xffffffffu) atomicMin(&s_lo, p);
        __syncthreads();
        live = s_lo;
        (void)lo;
    }
    // thread t takes splitters t * kPer .. + kPer - 1 and makes them non-decreasing with a
    // running max (an order the host's pass budget left incomplete — that frame re-renders
    // — must still give sorted splitters: the bucket search assumes them)
    constexpr int kPer = B / kBktThreads;
    __shared__ uint32_t s_wmax[4];
    uint32_t v[kPer], run = 0;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const uint32_t j = t * kPer + k;
        v[k] = live && j < (uint32_t)B - 2u ? (uint32_t)(sorted[bkt_split_pos<B>(j, live)] >> 32) : 0u;
        v[k] = min(v[k], 0xfffffffeu);
        run = max(run, v[k]);
        v[k] = run;
    }
    // inclusive max over the wave's threads, then over earlier waves
    const uint32_t lane = t & 63u, w = t >> 6;
    const uint32_t x = wave_incl_scan(run, OpMax{});
    if (lane == 63) s_wmax[w] = x;
    uint32_t before = wave_shr1(x);
    __syncthreads();
    for (uint32_t k = 0; k < w; k++) before = max(before, s_wmax[k]);
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const uint32_t j = t * kPer + k;
        if (j < (uint32_t)B - 2u) s_out[j] = max(before, v[k]);
    }
    if (t == 0) s_out[B - 2] = 0xffffffffu;
}

// Depth split, phase B: the summed-area table of the tiles phase A left unsaturated
// (a tile counts when any of its four blocks' flags is set; the flags of a tile are
// consecutive bytes), (tiles_y + 1) x (tiles_x + 1) words with a zero first row and
// column.  One workgroup: row prefix sums, then column prefix sums.
__global__ __launch_bounds__(256) void k_split_sat(const uint8_t* __restrict__ bflag, int tiles_x, int tiles_y,
                                                    uint32_t* __restrict__ sat, const uint32_t* __restrict__ gate) {
    GSR_GEOM_PRIO();
    if (*gate == 0u) return;
    const int w = tiles_x + 1;
    const uint32_t* tf = reinterpret_cast<const uint32_t*>(bflag);
    for (int y = (int)threadIdx.x; y <= tiles_y; y += 256) {
        uint32_t* row = sat + (size_t)y * (uint32_t)w;
        uint32_t run = 0;
        row[0] = 0;
        for (int x = 0; x < tiles_x; x++) {
            if (y > 0) run += tf[(size_t)(y - 1) * (uint32_t)tiles_x + (uint32_t)x] != 0u ? 1u : 0u;
            row[x + 1] = run;
        }
    }
    __syncthreads();
    for (int x = (int)threadIdx.x + 1; x <= tiles_x; x += 256) {
        uint32_t run = 0;
        for (int y = 1; y <= tiles_y; y++) {
            run += sat[(size_t)y * (uint32_t)w + (uint32_t)x];
            sat[(size_t)y * (uint32_t)w + (uint32_t)x] = run;
        }
    }
}

// Row pass, count: per workgroup (1024-Gaussian sub-chunks in depth order) the
// number of row items and of pairs per tile row; hist[row][g] and
// hist[256 + row][g].  Reads the rects in depth order (the payloads the depth
// sort carried, depth_sorted_rects).
__global__ __launch_bounds__(256) void k_bin_rows_count(uint32_t n, const uint32_t* __restrict__ pay0,
                                                         const uint32_t* __restrict__ pay1,
                                                         const uint32_t* __restrict__ dstats, int groups,
                                                         int tiles_y, uint32_t* __restrict__ hist, uint32_t base,
                                                         const uint32_t* __restrict__ gate,
                                                         const uint32_t* __restrict__ cut, int cut_mode,
                                                         const uint32_t* __restrict__ cut_n) {
    GSR_GEOM_PRIO();
    if (gate && *gate == 0u) return;   // depth split, phase B: every block saturated in phase A
    row_range(base, n, cut, cut_mode, cut_n);
    __shared__ uint32_t h_items[4][256], h_pairs[4][256];
    const uint32_t t = threadIdx.x, w = t >> 6;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        h_items[k][t] = 0;
        h_pairs[k][t] = 0;
    }
    __syncthreads();
    const uint32_t* srect = depth_sorted_rects(pay0, pay1, dstats) + base;
    const int chunk = (int)blockIdx.x;   // (XCD-contiguous chunks: 16.2 -> 18.7 us at config 3)
    uint64_t b, e;
    chunk_range(n, groups, chunk, kRowSources, b, e);
    for (uint64_t c0 = b; c0 < e; c0 += 1024) {
        uint64_t r[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint64_t j = c0 + t + 256 * k;
            r[k] = j < e ? unpack_rect(srect[j]) : kDeadRect;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            // difference arrays: +1 / +cols at the first row, -1 / -cols past the last
            if (rect_count(r[k])) {
                const uint32_t ty0 = (uint32_t)((r[k] >> 32) & 0xffffu), ty1 = (uint32_t)(r[k] >> 48);
                const uint32_t cols = rect_cols(r[k]);
                atomicAdd(&h_items[w][ty0], 1u);
                atomicAdd(&h_pairs[w][ty0], cols);
                if (ty1 < 255u) {
                    atomicSub(&h_items[w][ty1 + 1], 1u);
                    atomicSub(&h_pairs[w][ty1 + 1], cols);
                }
            }
        }
    }
    __syncthreads();
    // prefix over rows turns the differences into per-row counts (mod 2^32)
    uint32_t ti, tp;
    const uint32_t di = h_items[0][t] + h_items[1][t] + h_items[2][t] + h_items[3][t];
    const uint32_t dp = h_pairs[0][t] + h_pairs[1][t] + h_pairs[2][t] + h_pairs[3][t];
    __shared__ uint32_t scr[4];
    const uint32_t ci = block_exclusive_scan<uint32_t>(di, scr, ti) + di;
    const uint32_t cp = block_exclusive_scan<uint32_t>(dp, scr, tp) + dp;
    if (t < (uint32_t)tiles_y) {   // rows past the grid hold nothing: no scattered writes for them
        hist[t * (uint32_t)groups + chunk] = ci;
        hist[(256 + t) * (uint32_t)groups + chunk] = cp;
    }
}

// Row pass, scan: one workgroup per row.  Exclusive scan of the row's item
// counts over the workgroups (in place) and the row's totals.
__global__ __launch_bounds__(256) void k_bin_rows_scan(uint32_t* __restrict__ hist, int groups, int tiles_y,
                                                        uint32_t* __restrict__ row_items,
                                                        unsigned long long* __restrict__ row_pairs,
                                                        uint32_t* __restrict__ gate, int gate_mode) {
    GSR_GEOM_PRIO();
    // depth split: phase A clears the count of unsaturated blocks its blend raises;
    // phase B runs only when that count is not zero
    if (gate_mode == 1 && blockIdx.x == 0 && threadIdx.x == 0) *gate = 0u;
    if (gate_mode == 2 && *gate == 0u) return;
    __shared__ uint32_t scr[4];
    __shared__ unsigned long long scr64[4];
    const uint32_t r = blockIdx.x, t = threadIdx.x;
    if (r >= (uint32_t)tiles_y) {   // all 256 row totals are read downstream
        if (t == 0) {
            row_items[r] = 0;
            row_pairs[r] = 0;
        }
        return;
    }
    uint32_t* hi = hist + (size_t)r * (uint32_t)groups;
    const uint32_t* hp = hist + (size_t)(256 + r) * (uint32_t)groups;
    const int per = (groups + 255) / 256;
    const int b = (int)t * per;
    // all loads of the segment issued together (k_radix_scan)
    constexpr int kPerMax = kMaxSortGroups / 256;
    uint32_t v[kPerMax], local = 0;
    unsigned long long lp = 0;
#pragma unroll
    for (int k = 0; k < kPerMax; k++) {
        const bool in = k < per && b + k < groups;
        v[k] = in ? hi[b + k] : 0u;
        lp += in ? hp[b + k] : 0u;
        local += v[k];
    }
    uint32_t tot;
    uint32_t run = block_exclusive_scan<uint32_t>(local, scr, tot);
    unsigned long long ptot;
    block_exclusive_scan<unsigned long long>(lp, scr64, ptot);
#pragma unroll
    for (int k = 0; k < kPerMax; k++)
        if (k < per && b + k < groups) {
            hi[b + k] = run;
            run += v[k];
        }
    if (t == 0) {
        row_items[r] = tot;
        row_pairs[r] = ptot;
    }
}

// Row pass, scatter: the workgroup's Gaussians, 1024 at a time, expand into
// their row items; tiles of 256*ITEMS items are ranked by row and written in
// row runs to rows_out (positions >= cap are dropped; the frame then overflows
// and the column pass emits nothing).  The sorted tile holds only each item's
// source slot: the payload (index | tx0 << 32 | tx1 << 48) is rebuilt at the write.
template <int ITEMS, int BITS, bool RA>
__global__ __launch_bounds__(256, ITEMS == 4 ? 6 : 1) void k_bin_rows_scatter(const uint64_t* __restrict__ items0,
                                                           const uint64_t* __restrict__ items1,
                                                           const uint32_t* __restrict__ dstats,
                                                           const uint32_t* __restrict__ pay0,
                                                           const uint32_t* __restrict__ pay1, uint32_t n,
                                                           int groups, const uint32_t* __restrict__ hist,
                                                           const uint32_t* __restrict__ row_items,
                                                           const unsigned long long* __restrict__ row_pairs,
                                                           uint32_t cap, int tiles_y, uint64_t* __restrict__ rows_out,
                                                           const uint16_t* __restrict__ spans, uint32_t base,
                                                           const uint32_t* __restrict__ gate,
                                                           const uint32_t* __restrict__ cut, int cut_mode,
                                                           const uint32_t* __restrict__ cut_n,
                                                           const uint32_t* __restrict__ cstart) {
    GSR_GEOM_PRIO();
    if (gate && *gate == 0u) return;
    row_range(base, n, cut, cut_mode, cut_n);
    constexpr uint32_t kTile = 256u * ITEMS;
    // per source: exclusive start << 8 | first tile row; index
    __shared__ uint32_t s_ft[kRowSources], s_idx[kRowSources];
    // per source: packed rect (pack_rect) | tile row spans << 32 (no LDS beyond the
    // 8 B per source it always had: 6 workgroups per CU)
    __shared__ uint64_t s_rect[kRowSources];
    // s_own (source owners, read by the generation) and s_dl (the ranked tile: source
    // slot << 8 | row, written after the ranking) share storage: their lives do not overlap
    __shared__ uint32_t s_dl[kTile];
    uint16_t* const s_own = reinterpret_cast<uint16_t*>(s_dl);
    __shared__ uint32_t s_wmax[4];
    // s_dbase[d]: global position of the tile's first item of row d minus its tile slot
    __shared__ uint32_t s_wc[4][256], s_dbase[256], s_lbase[256], s_scr[4];
    __shared__ unsigned long long s_scr64[4];
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    uint64_t b, e;
    const int chunk = (int)blockIdx.x;
    if (cstart) {   // the chunks are the bucket sort's buckets (k_bkt_local counted them)
        b = min(cstart[chunk], n);
        e = min(cstart[chunk + 1], n);
    } else {
        chunk_range(n, groups, chunk, kRowSources, b, e);
    }
    const uint64_t* sorted = depth_sorted(items0, items1, dstats) + base;
    const uint32_t* srect = depth_sorted_rects(pay0, pay1, dstats) + base;
    // thread t owns sources 4t .. 4t+3 of a sub-chunk (source order): packed rect, index
    // and (by index) tile row spans; the first sub-chunk's (usually the only one) are
    // loaded before the base scan, so the dependent spans gather overlaps it (loading
    // every next sub-chunk ahead too holds 86 VGPRs: one wave per SIMD fewer)
    uint32_t prc[4], gix[4], spv[4];
    auto load_sources = [&](uint64_t c0) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint64_t j = c0 + 4 * t + i;
            prc[i] = j < e ? srect[j] : pack_rect(kDeadRect);
            gix[i] = j < e ? (uint32_t)sorted[j] : 0u;
        }
#pragma unroll
        for (int i = 0; i < 4; i++) spv[i] = spans && rect_rows(unpack_rect(prc[i])) ? spans[gix[i]] : 0u;
    };
    load_sources(b);
    uint32_t gb;   // row t's running global position (thread t owns row t)
    {
        uint32_t tot;
        gb = block_exclusive_scan<uint32_t>(row_items[t], s_scr, tot) +
             (t < (uint32_t)tiles_y ? hist[t * (uint32_t)groups + chunk] : 0u);
        unsigned long long ptot;
        block_exclusive_scan<unsigned long long>(row_pairs[t], s_scr64, ptot);
        if (ptot > cap || b >= e) return;   // uniform: overflow frames stop here
    }
    for (uint64_t c0 = b; c0 < e; c0 += kRowSources) {
        if (c0 != b) load_sources(c0);
        uint32_t cnt[4], start[4], ty0v[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            s_idx[4 * t + i] = gix[i];
            cnt[i] = rect_rows(unpack_rect(prc[i]));
            ty0v[i] = (prc[i] >> 16) & 0xffu;
        }
#pragma unroll
        for (int i = 0; i < ITEMS; i++) s_own[t * ITEMS + i] = 0;
        const uint32_t total = bin_source_starts<4>(cnt, start, ty0v, s_ft, s_scr);
#pragma unroll
        for (int i = 0; i < 4; i++)   // read after bin_tile_owners' barriers
            s_rect[4 * t + i] = (uint64_t)prc[i] | ((uint64_t)spv[i] << 32);
        uint32_t carry = 0;
        for (uint32_t tb = 0; tb < total; tb += kTile) {
            const uint32_t tn = min(kTile, total - tb);
            bin_tile_owners<ITEMS, 4>(cnt, start, tb, tn, s_own, carry, s_wmax);
            uint32_t dig[ITEMS], pos[ITEMS], src[ITEMS];
#pragma unroll
            for (int k = 0; k < ITEMS; k++) {
                const uint32_t el = min(w * 64 * ITEMS + k * 64 + lane, tn - 1);
                const uint32_t l = (uint32_t)s_own[el] - 1u;
                src[k] = l;
                const uint32_t ft = s_ft[l];
                dig[k] = (ft & 0xffu) + (tb + el - (ft >> 8));   // ty0 + row
            }
            const uint32_t tcount = bin_rank_tile<ITEMS, BITS, RA>(dig, tn, pos, s_wc, s_lbase, s_scr);
            s_dbase[t] = gb - s_lbase[t];   // this thread's own scan output
#pragma unroll
            for (int k = 0; k < ITEMS; k++) {
                const uint32_t el = w * 64 * ITEMS + k * 64 + lane;
                if (el < tn) s_dl[pos[k]] = (src[k] << 8) | dig[k];
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < ITEMS; k++) {
                const uint32_t q = t + 256 * k;
                const uint32_t qc = min(q, tn - 1);
                const uint32_t x = s_dl[qc];
                const uint32_t d = x & 0xffu, l = x >> 8;
                const uint32_t dst = s_dbase[d] + qc;
                const uint64_t r = s_rect[l];
                uint32_t x0 = (uint32_t)(r & 0xffu), x1 = (uint32_t)((r >> 8) & 0xffu);
                const uint32_t ro = d - (uint32_t)((r >> 16) & 0xffu);   // row within the rect
                if (ro < 4u) {
                    // tile row spans: columns [x0 + left, x1 - right]; an empty row gets the
                    // empty range (1, 0), which the column pass counts and expands to nothing
                    const uint32_t sp = (uint32_t)(r >> (32u + 4u * ro)) & 15u;
                    const int c0 = (int)(x0 + (sp & 3u)), c1 = (int)x1 - (int)(sp >> 2);
                    x0 = c0 <= c1 ? (uint32_t)c0 : 1u;
                    x1 = c0 <= c1 ? (uint32_t)c1 : 0u;
                }
                if (q < tn && dst < cap) rows_out[dst] = (uint64_t)s_idx[l] | ((uint64_t)x0 << 32) | ((uint64_t)x1 << 48);
            }
            __syncthreads();
            gb += tcount;
#pragma unroll
            for (int i = 0; i < ITEMS; i++) s_own[t * ITEMS + i] = 0;   // owners of the next tile start cleared
            __syncthreads();
        }
    }
}

// Row geometry of the column pass, rebuilt by each workgroup from the row
// totals: item base and count per row, first chunk per row (chunks of
// CH items never cross a row), chunk total, pair base per row, P.
// (PB: also the pair base per row — only the column scan needs it.)
template <bool PB>
struct ColPlan {
    uint32_t rbase[256], rcnt[256], chbase[257];
    unsigned long long pbase[PB ? 256 : 1];
};

template <uint32_t CH, bool PB>
__device__ __forceinline__ unsigned long long col_plan(const uint32_t* __restrict__ row_items,
                                                       const unsigned long long* __restrict__ row_pairs,
                                                       ColPlan<PB>& pl, uint32_t* s_scr,
                                                       unsigned long long* s_scr64) {
    const uint32_t t = threadIdx.x;
    const uint32_t cnt = row_items[t];
    uint32_t tot;
    pl.rbase[t] = block_exclusive_scan<uint32_t>(cnt, s_scr, tot);
    pl.rcnt[t] = cnt;
    pl.chbase[t] = block_exclusive_scan<uint32_t>((cnt + CH - 1) / CH, s_scr, tot);
    if (t == 255) pl.chbase[256] = tot;
    unsigned long long ptot;
    const unsigned long long pb = block_exclusive_scan<unsigned long long>(row_pairs[t], s_scr64, ptot);
    if (PB) pl.pbase[t] = pb;
    __syncthreads();
    return ptot;
}

// Row of chunk c: the last row whose first chunk is <= c (empty rows own none).
template <bool PB>
__device__ __forceinline__ uint32_t col_chunk_row(const ColPlan<PB>& pl, uint32_t c) {
    uint32_t l = 0;
#pragma unroll
    for (uint32_t st = 128; st >= 1; st >>= 1)
        if (pl.chbase[l + st] <= c) l += st;
    return l;
}

// Column pass, count: per chunk, pairs per tile column -> cbins[chunk][col].
template <uint32_t CH>
__global__ __launch_bounds__(256) void k_bin_cols_count(const uint64_t* __restrict__ rows_in,
                                                         const uint32_t* __restrict__ row_items,
                                                         const unsigned long long* __restrict__ row_pairs,
                                                         uint32_t cap, int tiles_x, uint32_t* __restrict__ cbins,
                                                         const uint32_t* __restrict__ gate) {
    GSR_GEOM_PRIO();
    if (gate && *gate == 0u) return;
    __shared__ ColPlan<false> pl;
    __shared__ uint32_t h[4][256], s_scr[4];
    __shared__ unsigned long long s_scr64[4];
    const uint32_t t = threadIdx.x, w = t >> 6;
    if (col_plan<CH>(row_items, row_pairs, pl, s_scr, s_scr64) > cap) return;
    const uint32_t nch = pl.chbase[256];
    for (uint32_t c = blockIdx.x; c < nch; c += gridDim.x) {
#pragma unroll
        for (int k = 0; k < 4; k++) h[k][t] = 0;
        __syncthreads();
        const uint32_t r = col_chunk_row(pl, c);
        const uint32_t ib = pl.rbase[r] + (c - pl.chbase[r]) * CH;
        const uint32_t ie = min(ib + CH, pl.rbase[r] + pl.rcnt[r]);
        // difference arrays: +1 at the first column, -1 past the last (all of a thread's
        // loads issued before its first LDS update)
        constexpr int PER = CH / 256;
        uint64_t its[PER];
#pragma unroll
        for (int k = 0; k < PER; k++) its[k] = ib + t + 256 * k < ie ? rows_in[ib + t + 256 * k] : 0ull;
#pragma unroll
        for (int k = 0; k < PER; k++)
            if (ib + t + 256 * k < ie) {
                const uint32_t tx0 = (uint32_t)((its[k] >> 32) & 0xffffu), tx1 = (uint32_t)(its[k] >> 48);
                atomicAdd(&h[w][tx0], 1u);
                if (tx1 < 255u) atomicSub(&h[w][tx1 + 1], 1u);
            }
        __syncthreads();
        const uint32_t dsum = h[0][t] + h[1][t] + h[2][t] + h[3][t];
        uint32_t tot;
        const uint32_t cnt = block_exclusive_scan<uint32_t>(dsum, s_scr, tot) + dsum;   // mod 2^32
        if (t < (uint32_t)tiles_x) cbins[(size_t)c * 256 + t] = cnt;
    }
}

// Column pass, scan: one workgroup per row.  Exclusive scan of each column's
// chunk counts over the row's chunks (in place), then the row's tiles: start =
// row pair base + exclusive scan over columns; ranges = {~start, end} (zero =
// empty).  Overflowed frames (P > cap) get empty ranges.  Workgroup 0 publishes
// the frame's pair statistics.
template <uint32_t CH>
__global__ __launch_bounds__(256) void k_bin_cols_scan(const uint32_t* __restrict__ row_items,
                                                        const unsigned long long* __restrict__ row_pairs,
                                                        uint32_t cap, int tiles_x, uint32_t* __restrict__ cbins,
                                                        uint2* __restrict__ ranges, Stats* __restrict__ st,
                                                        Stats* host_st, const uint32_t* __restrict__ dstats,
                                                        int passes_launched, const uint32_t* __restrict__ gate,
                                                        uint32_t* fstatus) {
    GSR_GEOM_PRIO();
    if (gate && *gate == 0u) return;
    __shared__ ColPlan<true> pl;
    __shared__ uint32_t s_scr[4];
    __shared__ unsigned long long s_scr64[4];
    const uint32_t t = threadIdx.x, r = blockIdx.x;
    const unsigned long long P = col_plan<CH>(row_items, row_pairs, pl, s_scr, s_scr64);
    if (r == 0 && t == 0)
        publish_pair_stats(P, cap, st, host_st, dstats ? (uint32_t)depth_passes_run(dstats) : 0u,
                           (uint32_t)passes_launched, fstatus, gate == nullptr);
    uint32_t run = 0;
    if (P <= cap && t < (uint32_t)tiles_x) {
        // 32 chunks per step: the loads are issued together, not one round trip per chunk
        // (a row of the 5M-Gaussian frame has ~75 chunks: 3 round trips instead of 10)
        const uint32_t c1 = pl.chbase[r + 1];
        for (uint32_t c0 = pl.chbase[r]; c0 < c1; c0 += 32) {
            uint32_t v[32];
#pragma unroll
            for (int k = 0; k < 32; k++) v[k] = c0 + k < c1 ? cbins[(size_t)(c0 + k) * 256 + t] : 0u;
#pragma unroll
            for (int k = 0; k < 32; k++)
                if (c0 + k < c1) {
                    cbins[(size_t)(c0 + k) * 256 + t] = run;
                    run += v[k];
                }
        }
    }
    uint32_t tot;
    const uint32_t excl = block_exclusive_scan<uint32_t>(run, s_scr, tot);
    if (t < (uint32_t)tiles_x) {
        const uint32_t start = (uint32_t)pl.pbase[r] + excl;
        ranges[r * (uint32_t)tiles_x + t] = run ? make_uint2(~start, start + run) : make_uint2(0u, 0u);
    }
}

// Column pass, scatter: per chunk, its row items expand into one value per
// covered column; tiles of 256*ITEMS values are ranked by column and written in
// column runs at tile start + chunk offset.
template <int ITEMS, int BITS, bool RA, uint32_t CH>
__global__ __launch_bounds__(256) void k_bin_cols_scatter(const uint64_t* __restrict__ rows_in,
                                                           const uint32_t* __restrict__ row_items,
                                                           const unsigned long long* __restrict__ row_pairs,
                                                           uint32_t cap, int tiles_x,
                                                           const uint32_t* __restrict__ cbins,
                                                           const uint2* __restrict__ ranges,
                                                           uint32_t* __restrict__ vals,
                                                           const uint32_t* __restrict__ gate) {
    GSR_GEOM_PRIO();
    if (gate && *gate == 0u) return;
    constexpr uint32_t kTile = 256u * ITEMS;
    __shared__ ColPlan<false> pl;
    // per source (row item of the chunk): exclusive start << 8 | first column; index
    __shared__ uint32_t s_ft[CH], s_idx[CH];
    __shared__ uint16_t s_own[kTile];
    __shared__ uint32_t s_dl[kTile];   // the ranked tile: source slot << 8 | column
    __shared__ uint32_t s_wmax[4];
    // s_dbase[d]: global position of the tile's first value of column d minus its tile slot
    __shared__ uint32_t s_wc[4][256], s_dbase[256], s_lbase[256], s_scr[4];
    __shared__ unsigned long long s_scr64[4];
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    if (col_plan<CH>(row_items, row_pairs, pl, s_scr, s_scr64) > cap) return;
    const uint32_t nch = pl.chbase[256];
    for (uint32_t c = blockIdx.x; c < nch; c += gridDim.x) {
        const uint32_t r = col_chunk_row(pl, c);
        const uint32_t ib = pl.rbase[r] + (c - pl.chbase[r]) * CH;
        const uint32_t m = min(CH, pl.rbase[r] + pl.rcnt[r] - ib);
        // column t's running global position (thread t owns column t)
        uint32_t gb = t < (uint32_t)tiles_x ? ~ranges[r * (uint32_t)tiles_x + t].x + cbins[(size_t)c * 256 + t] : 0u;
        // thread t owns row items PER*t .. PER*t + PER-1 of the chunk (source order)
        constexpr int PER = CH / 256;
        uint32_t cnt[PER], start[PER], tx0v[PER];
#pragma unroll
        for (int i = 0; i < PER; i++) {
            const uint32_t j = PER * t + i;
            const uint64_t it = j < m ? rows_in[ib + j] : 0ull;
            const uint32_t tx0 = (uint32_t)((it >> 32) & 0xffffu);
            cnt[i] = j < m ? (uint32_t)(it >> 48) - tx0 + 1u : 0u;
            tx0v[i] = tx0 & 0xffu;
            s_idx[j] = (uint32_t)it;
        }
#pragma unroll
        for (int i = 0; i < ITEMS; i++) s_own[t * ITEMS + i] = 0;
        const uint32_t total = bin_source_starts<PER>(cnt, start, tx0v, s_ft, s_scr);
        uint32_t carry = 0;
        for (uint32_t tb = 0; tb < total; tb += kTile) {
            const uint32_t tn = min(kTile, total - tb);
            bin_tile_owners<ITEMS, PER>(cnt, start, tb, tn, s_own, carry, s_wmax);
            uint32_t dig[ITEMS], pos[ITEMS], src[ITEMS];
#pragma unroll
            for (int k = 0; k < ITEMS; k++) {
                const uint32_t el = min(w * 64 * ITEMS + k * 64 + lane, tn - 1);
                const uint32_t l = (uint32_t)s_own[el] - 1u;
                src[k] = l;
                const uint32_t ft = s_ft[l];
                dig[k] = (ft & 0xffu) + (tb + el - (ft >> 8));
            }
            const uint32_t tcount = bin_rank_tile<ITEMS, BITS, RA>(dig, tn, pos, s_wc, s_lbase, s_scr);
            s_dbase[t] = gb - s_lbase[t];   // this thread's own scan output
#pragma unroll
            for (int i = 0; i < ITEMS; i++) s_own[t * ITEMS + i] = 0;   // for the next tile (rank barriers passed)
#pragma unroll
            for (int k = 0; k < ITEMS; k++) {
                const uint32_t el = w * 64 * ITEMS + k * 64 + lane;
                if (el < tn) s_dl[pos[k]] = (src[k] << 8) | dig[k];
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < ITEMS; k++) {
                const uint32_t q = t + 256 * k;
                const uint32_t qc = min(q, tn - 1);
                const uint32_t x = s_dl[qc];
                const uint32_t v = s_idx[x >> 8];
                const uint32_t dst = s_dbase[x & 0xffu] + qc;
                if (q < tn) vals[dst] = v;
            }
            __syncthreads();
            gb += tcount;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------ live partition
//
// Stable partition of the preprocess items ahead of the global depth sort
// (GSR_TUNE_DEPTH_COMPACT): visible items (key != 0xFFFFFFFF) first, in index
// order, then the culled ones, in index order.  The full sort puts the culled
// items last in index order anyway (their key is the maximum, ties by index), so
// sorting only the visible prefix (n_dev = the visible count) gives the same
// order.  The visible items' rect payloads go to pay0 (pass 0 reads them there).
// The culled tail is written to `out` only, with the dead rect in both payload
// buffers at the same positions (the passes never touch the tail, and which buffer
// ends depth-ordered is decided on the device); the binning never reads items whose
// rect is dead, and gsr_read_depth_order takes the tail from `out`.  Three launches: per-chunk
// visible counts, their exclusive scan (+ total), the scatter.
__global__ __launch_bounds__(256) void k_part_count(const uint64_t* __restrict__ in, uint32_t n, int groups,
                                                     uint32_t* __restrict__ counts) {
    GSR_GEOM_PRIO();
    __shared__ uint32_t s_scr[4];
    uint64_t b, e;
    chunk_range(n, groups, blockIdx.x, 256, b, e);
    uint32_t c = 0;
    for (uint64_t i = b + threadIdx.x; i < e; i += 256) c += (uint32_t)(in[i] >> 32) != 0xffffffffu ? 1u : 0u;
    uint32_t tot;
    (void)block_exclusive_scan<uint32_t>(c, s_scr, tot);
    if (threadIdx.x == 0) counts[blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void k_part_scan(uint32_t* __restrict__ counts, int groups,
                                                    uint32_t* __restrict__ n_live) {
    GSR_GEOM_PRIO();
    __shared__ uint32_t s_scr[4];
    const int per = (groups + 255) / 256;
    const int b = (int)threadIdx.x * per;
    uint32_t local = 0;
    for (int k = 0; k < per; k++)
        if (b + k < groups) local += counts[b + k];
    uint32_t total;
    uint32_t run = block_exclusive_scan<uint32_t>(local, s_scr, total);
    for (int k = 0; k < per; k++)
        if (b + k < groups) {
            const uint32_t v = counts[b + k];
            counts[b + k] = run;
            run += v;
        }
    if (threadIdx.x == 0) *n_live = total;
}

__global__ __launch_bounds__(256) void k_part_scatter(const uint64_t* __restrict__ in, uint32_t n, int groups,
                                                       const uint32_t* __restrict__ offs,
                                                       const uint32_t* __restrict__ n_live,
                                                       uint64_t* __restrict__ out,
                                                       const uint32_t* __restrict__ rect,
                                                       uint32_t* __restrict__ pay0, uint32_t* __restrict__ pay1) {
    GSR_GEOM_PRIO();
    __shared__ uint32_t s_w[4];
    uint64_t b, e;
    chunk_range(n, groups, blockIdx.x, 256, b, e);
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    const uint64_t lt = lane ? (~0ull >> (64 - lane)) : 0ull;
    uint32_t live_base = offs[blockIdx.x];
    // culled items before this chunk = b - visible items before it
    uint32_t dead_base = *n_live + (uint32_t)(b - live_base);
    for (uint64_t c0 = b; c0 < e; c0 += 256) {
        const uint64_t i = c0 + t;
        const bool valid = i < e;
        const uint64_t v = valid ? in[i] : 0ull;
        const bool live = valid && (uint32_t)(v >> 32) != 0xffffffffu;
        const bool dead = valid && !live;
        const uint64_t bl = __ballot(live), bd = __ballot(dead);
        if (lane == 0) s_w[w] = (uint32_t)__popcll(bl) | ((uint32_t)__popcll(bd) << 16);
        __syncthreads();
        uint32_t lb = 0, db = 0, ltot = 0, dtot = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            const uint32_t x = s_w[k];
            if (k < w) {
                lb += x & 0xffffu;
                db += x >> 16;
            }
            ltot += x & 0xffffu;
            dtot += x >> 16;
        }
        if (live) {
            const uint32_t q = live_base + lb + (uint32_t)__popcll(bl & lt);
            out[q] = v;
            pay0[q] = rect[(uint32_t)v];   // pass 0 reads the payloads from pay0
        }
        if (dead) {
            const uint32_t q = dead_base + db + (uint32_t)__popcll(bd & lt);
            out[q] = v;
            pay0[q] = pack_rect(kDeadRect);   // the sort's result parity is decided on the device
            pay1[q] = pack_rect(kDeadRect);
        }
        live_base += ltot;
        dead_base += dtot;
        __syncthreads();
    }
}

// ------------------------------------------------------------------ standalone sort ABI helpers

// (u32(key) << 32 | i): the reference sorts int keys as unsigned 8-bit digits
// over all 32 bits (onesweep.cu:190-250, numPasses = 4).
__global__ void k_items_from_keys(const int* __restrict__ keys, uint32_t n, uint64_t* __restrict__ items) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) items[i] = ((uint64_t)(uint32_t)keys[i] << 32) | i;
}

__global__ void k_keys_from_items(const uint64_t* __restrict__ items, uint32_t n, int* __restrict__ keys) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) keys[i] = (int)(uint32_t)(items[i] >> 32);
}

// Stage items for lightWeightGaussian records: (bits [shift, shift+32) of
// radix_id << 32 | position).  src_perm (nullable) maps position -> record.
__global__ void k_items_from_lwg(const gsr_lwg* __restrict__ rec, const uint64_t* __restrict__ src_perm,
                                 uint32_t n, int shift, uint32_t mask, uint64_t* __restrict__ items) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = src_perm ? (uint32_t)src_perm[i] : i;
    const uint32_t k = (uint32_t)(rec[r].radix_id >> shift) & mask;
    items[i] = ((uint64_t)k << 32) | i;
}

__global__ void k_gather_lwg(const gsr_lwg* __restrict__ in, const uint64_t* __restrict__ stage1,
                             const uint64_t* __restrict__ stage2, uint32_t n, gsr_lwg* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t r = (uint32_t)stage2[i];
    if (stage1) r = (uint32_t)stage1[r];
    out[i] = in[r];
}

// gsr_alpha_take_min_x on the device, one opacity per thread (tests).
__global__ void k_xs_probe(const float* __restrict__ op, int n, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = gsr_alpha_take_min_x(op[i]);
}

}  // namespace

// ------------------------------------------------------------------ launchers

hipError_t launch_aos_to_soa(const gsr_gaussian* aos, int64_t n, float* arrays, int64_t stride,
                             hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_aos_to_soa, dim3(grid_for(n, 256)), dim3(256), 0, s, aos, n, arrays, stride);
    return hipGetLastError();
}

hipError_t launch_preprocess(const float* arrays, int64_t stride, int64_t n, const Frame& fr,
                             uint4* rec, uint64_t* items, uint64_t* rect, bool packed, bool four_d, bool sh3,
                             float t, hipStream_t s, uint16_t* spans, const RecSplit* rsp) {
    if (n <= 0) return hipSuccess;
    const RecSplit rs = rsp ? *rsp : RecSplit{0, nullptr, nullptr, nullptr};
    if ((rs.mode == 1 && (!rs.kcut || !rs.kcut_frame || spans)) || (rs.mode == 2 && !rs.kcut_frame) || rs.mode < 0 ||
        rs.mode > 2)
        return hipErrorInvalidValue;
    const dim3 g(grid_for(n, 256));
    const int pk = packed ? 1 : 0;
    if (four_d)
        hipLaunchKernelGGL((k_preprocess<true, false>), g, dim3(256), 0, s, arrays, stride, n, fr, rec, items, rect,
                           pk, packed ? spans : nullptr, t, rs);
    else if (sh3)
        hipLaunchKernelGGL((k_preprocess<false, true>), g, dim3(256), 0, s, arrays, stride, n, fr, rec, items, rect,
                           pk, packed ? spans : nullptr, t, rs);
    else
        hipLaunchKernelGGL((k_preprocess<false, false>), g, dim3(256), 0, s, arrays, stride, n, fr, rec, items, rect,
                           pk, packed ? spans : nullptr, t, rs);
    return hipGetLastError();
}

hipError_t launch_preprocess_multi(const float* arrays, int64_t stride, int64_t n, int nc, const Frame* const* fr,
                                   const PreTargets* out, bool sh3, hipStream_t s) {
    if (nc < 2 || nc > kPreMultiMax) return hipErrorInvalidValue;
    if (n <= 0) return hipSuccess;
    const dim3 g(grid_for(n, 256));
    auto go = [&](auto tag) {
        constexpr int NC = decltype(tag)::value;
        PreMulti<NC> m;
        for (int c = 0; c < NC; c++) {
            m.fr[c] = *fr[c];
            m.out[c] = PreOut{out[c].rec, out[c].items, out[c].rect, out[c].packed ? out[c].spans : nullptr,
                              out[c].packed ? 1 : 0};
        }
        if (sh3)
            hipLaunchKernelGGL((k_preprocess_multi<true, NC>), g, dim3(256), 0, s, arrays, stride, n, m);
        else
            hipLaunchKernelGGL((k_preprocess_multi<false, NC>), g, dim3(256), 0, s, arrays, stride, n, m);
    };
    if (nc == 2) go(std::integral_constant<int, 2>{});
    else if (nc == 3) go(std::integral_constant<int, 3>{});
    else go(std::integral_constant<int, 4>{});
    return hipGetLastError();
}

// A filtered pass 0 ranks by the rect payloads it reads at each position (rect_direct).
static bool carry_ok(const uint32_t* pay0, int rect_direct) { return pay0 != nullptr && rect_direct > 0; }

template <int ITEMS, bool RA>
static void radix_pass(const uint64_t* in, uint64_t* out, const uint32_t* n_dev, uint32_t n_host, int shift,
                       int bits, int groups, uint32_t* hist, uint32_t* totals, uint2* ranges, uint32_t* dstats,
                       int pass, const uint32_t* rect, int rect_direct, uint32_t* pay0, uint32_t* pay1,
                       hipStream_t s, SortRange sr) {
    const uint32_t mask = (1u << bits) - 1u;
    // rect payloads (binning): pass p reads pay[p & 1] (pass 0: rect, or pay[0] when
    // rect_direct < 0 — the live partition wrote it) and writes pay[(p + 1) & 1]
    const uint32_t* pay_in = pay0 && (pass > 0 || rect_direct < 0) ? ((pass & 1) ? pay1 : pay0) : nullptr;
    uint32_t* pay_out = pay0 ? ((pass & 1) ? pay0 : pay1) : nullptr;
    with_bool(sr.filter != 0, [&](auto filt) {
        constexpr bool FILT = decltype(filt)::value;
        hipLaunchKernelGGL((k_radix_upsweep<ITEMS, FILT>), dim3(groups), dim3(kSortThreads), 0, s, in, n_dev, n_host,
                           shift, mask, groups, hist, dstats, pass, sr);
        hipLaunchKernelGGL(k_radix_scan, dim3(256), dim3(256), 0, s, hist, groups, totals,
                           static_cast<const uint32_t*>(dstats), pass, sr.gate);
        hipLaunchKernelGGL((k_radix_downsweep<ITEMS, RA, FILT>), dim3(groups), dim3(kSortThreads), 0, s, in, out, n_dev,
                           n_host, shift, bits, groups, hist, totals, ranges, static_cast<const uint32_t*>(dstats), pass,
                           rect, rect_direct > 0 ? 1 : 0, pay_in, pay_out, sr);
    });
}

hipError_t launch_radix_pass(const uint64_t* in, uint64_t* out, const uint32_t* n_dev, uint32_t n_host,
                             int shift, int bits, int groups, int items, uint32_t* hist, uint32_t* totals,
                             uint2* ranges, hipStream_t s, uint32_t* dstats, int pass, const uint32_t* rect,
                             int rect_direct, uint32_t* pay0, uint32_t* pay1, bool rank_atomic,
                             const uint32_t* base_dev, const uint32_t* gate, const SortFilter* f) {
    if ((rect == nullptr) != (pay0 == nullptr) || (pay0 == nullptr) != (pay1 == nullptr))
        return hipErrorInvalidValue;
    const int filter = f ? f->mode : 0;
    if (filter < 0 || filter > 2 || (filter && (pass != 0 || !f->kcut || n_dev || (filter == 2) != (base_dev != nullptr))))
        return hipErrorInvalidValue;
    if (base_dev && !filter && (n_dev || rect_direct > 0)) return hipErrorInvalidValue;
    if (filter && !carry_ok(pay0, rect_direct)) return hipErrorInvalidValue;
    const SortRange sr{base_dev, gate, filter ? f->kcut : nullptr, filter, filter ? f->count_out : nullptr,
                       filter == 1 ? f->kcut_copy : nullptr, filter == 2 ? f->sat : nullptr, f ? f->sat_w : 0,
                       filter == 2 && f->sat ? rect : nullptr, f && !filter ? f->count : nullptr};
    // 16 items per thread always rank with ballots, one tile per workgroup
    // (k_radix_downsweep): a grid too small for that sorts 8 per thread
    if (items == 16 && (uint64_t)groups * kSortTile < (uint64_t)n_host) items = 8;
    if (items == 4 || items == 8)
        with_bool(rank_atomic, [&](auto ra) {
            constexpr bool RA = decltype(ra)::value;
            if (items == 4)
                radix_pass<4, RA>(in, out, n_dev, n_host, shift, bits, groups, hist, totals, ranges, dstats, pass, rect,
                                  rect_direct, pay0, pay1, s, sr);
            else
                radix_pass<8, RA>(in, out, n_dev, n_host, shift, bits, groups, hist, totals, ranges, dstats, pass, rect,
                                  rect_direct, pay0, pay1, s, sr);
        });
    else
        radix_pass<16, false>(in, out, n_dev, n_host, shift, bits, groups, hist, totals, ranges, dstats, pass, rect,
                              rect_direct, pay0, pay1, s, sr);
    return hipGetLastError();
}

template <int B>
static void bucket_sort_b(const uint64_t* in, uint64_t* items0, uint64_t* items1, uint32_t n, int groups,
                          const uint32_t* s_in, uint32_t* s_out, uint32_t* hist, uint32_t* totals,
                          const uint32_t* rect, uint32_t* pay0, uint32_t* pay1, bool rank_atomic, uint32_t cap,
                          unsigned int* over_host, hipStream_t s, int row_tiles_y, uint4* rec) {
    // fused row-pass count: the row hist overwrites the bucket hist, which only the scatter reads
    // (grid B with it: the last bucket is the row pass's last chunk, k_bkt_local)
    const RowHist rh{row_tiles_y > 0 ? hist : nullptr, B, row_tiles_y};
    const int local_grid = row_tiles_y > 0 ? B : B - 1;
    uint32_t* bstart = totals + B;   // B + 2 words after the totals
    constexpr int kScTh = B >= 512 ? 512 : kBktThreads;   // k_bkt_scatter's workgroup size
    hipLaunchKernelGGL(k_bkt_count<B>, dim3(groups), dim3(kBktThreads), 0, s, in, n, s_in, groups, hist,
                       static_cast<uint16_t*>(nullptr));
    hipLaunchKernelGGL(k_bkt_scan<B>, dim3(B / 64), dim3(1024), 0, s, hist, groups, totals);
    with_bool(rank_atomic, [&](auto ra) {
        constexpr bool RA = decltype(ra)::value;
        hipLaunchKernelGGL((k_bkt_scatter<B, RA, kScTh, false>), dim3(groups), dim3(kScTh), 0, s, in, items0, n, s_in,
                           groups, hist, static_cast<const uint32_t*>(totals), rect, pay0, bstart, rec,
                           static_cast<const uint16_t*>(nullptr));
        hipLaunchKernelGGL((k_bkt_local<B, RA>), dim3(local_grid), dim3(kBktThreads), 0, s, items0, items1, pay0,
                           pay1, bstart, s_in, s_out, cap, over_host, rh, static_cast<const uint4*>(rec));
    });
}

hipError_t launch_bucket_sort(const uint64_t* in, uint64_t* items0, uint64_t* items1, uint32_t n, int buckets,
                              int groups, const uint32_t* s_in, uint32_t* s_out, uint32_t* hist, uint32_t* totals,
                              const uint32_t* rect, uint32_t* pay0, uint32_t* pay1, bool rank_atomic, uint32_t cap,
                              unsigned int* over_host, hipStream_t s, int row_tiles_y, uint4* rec) {
    if (groups < 1 || groups > kBktMaxGroups || (int64_t)groups * buckets > 256 * (int64_t)kMaxSortGroups || cap < 1 ||
        cap > kBktCap ||
        in == items0 || !rect || !pay0 || !pay1 || !rec)   // in may be items1: the scratch is used after the scatter
        return hipErrorInvalidValue;
    if (n == 0 || row_tiles_y > 256 || (int64_t)512 * buckets > 256 * (int64_t)kMaxSortGroups)
        return n == 0 ? hipSuccess : hipErrorInvalidValue;
    switch (buckets) {
    case 256: bucket_sort_b<256>(in, items0, items1, n, groups, s_in, s_out, hist, totals, rect, pay0, pay1, rank_atomic, cap, over_host, s, row_tiles_y, rec); break;
    case 512: bucket_sort_b<512>(in, items0, items1, n, groups, s_in, s_out, hist, totals, rect, pay0, pay1, rank_atomic, cap, over_host, s, row_tiles_y, rec); break;
    case 1024: bucket_sort_b<1024>(in, items0, items1, n, groups, s_in, s_out, hist, totals, rect, pay0, pay1, rank_atomic, cap, over_host, s, row_tiles_y, rec); break;
    case 2048: bucket_sort_b<2048>(in, items0, items1, n, groups, s_in, s_out, hist, totals, rect, pay0, pay1, rank_atomic, cap, over_host, s, row_tiles_y, rec); break;
    case 4096: bucket_sort_b<4096>(in, items0, items1, n, groups, s_in, s_out, hist, totals, rect, pay0, pay1, rank_atomic, cap, over_host, s, row_tiles_y, rec); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// kBigBuckets buckets, each sorted by one kBbThreads-thread workgroup.  The scatter's tile is
// staged (bucket runs written coalesced), barrier-lean (52.0 -> 50.2 us at config 3 orbit) and
// writes 12-B records (16-B: 51.7 -> 50.5 us); the eight-barrier tile, 16-B records and the
// unstaged scatter measured slower (profiles/r06k_big_buckets_c3_orbit.txt, DESIGN.md
// section 3).
hipError_t launch_bucket_sort_big(const uint64_t* in, uint64_t* items0, uint64_t* items1, uint32_t n, int buckets,
                                  int groups, const uint32_t* s_in, uint32_t* s_out, uint32_t* hist, uint32_t* totals,
                                  const uint32_t* rect, uint32_t* pay0, uint32_t* pay1, bool rank_atomic, uint32_t cap,
                                  unsigned int* over_host, hipStream_t s, uint4* rec) {
    constexpr int B = kBigBuckets;
    if (buckets != B || groups < 1 || groups > kBigBucketGroups ||
        (int64_t)groups * buckets > 256 * (int64_t)kMaxSortGroups || cap < 1 || in == items0 || !rect || !pay0 ||
        !pay1 || !rec)
        return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    uint32_t* bstart = totals + B;          // B + 2 words after the totals
    uint32_t* left = totals + 2 * B + 2;    // per bucket: k_bbk_local left it to k_bkt_local
    const RowHist none{nullptr, B, 0};
    // the count hands each item's bucket to the scatter (u16 in pay1, free until the second
    // launch), which then skips its own splitter search
    uint16_t* bid = reinterpret_cast<uint16_t*>(pay1);
    hipLaunchKernelGGL(k_bkt_count<B>, dim3(groups), dim3(kBktThreads), 0, s, in, n, s_in, groups, hist, bid);
    hipLaunchKernelGGL(k_bkt_scan_g, dim3(B / 16), dim3(1024), 0, s, hist, groups, totals);
    with_bool(rank_atomic, [&](auto ra) {
        constexpr bool RA = decltype(ra)::value;
        hipLaunchKernelGGL((k_bkt_scatter<B, RA, 512, true>), dim3(groups), dim3(512), 0, s, in, items0, n, s_in,
                           groups, hist, static_cast<const uint32_t*>(totals), rect, pay0, bstart, rec,
                           static_cast<const uint16_t*>(bid));
        hipLaunchKernelGGL(k_bbk_local<RA>, dim3(B - 1), dim3(kBbThreads), 0, s, items0, pay0,
                           static_cast<const uint32_t*>(bstart), s_in, s_out, cap, static_cast<const uint4*>(rec), left);
        hipLaunchKernelGGL((k_bkt_local<B, RA, true>), dim3(B - 1), dim3(kBktThreads), 0, s, items0, items1, pay0,
                           pay1, bstart, s_in, s_out, min(cap, kBktCap), over_host, none,
                           static_cast<const uint4*>(rec), static_cast<const uint32_t*>(left));
    });
    return hipGetLastError();
}

hipError_t launch_bkt_splitters(const uint64_t* items0, const uint64_t* items1, const uint32_t* dstats, uint32_t n,
                                const uint32_t* live_dev, int buckets, uint32_t* s_out, hipStream_t s) {
    switch (buckets) {
    case 256: hipLaunchKernelGGL(k_bkt_splitters<256>, dim3(1), dim3(kBktThreads), 0, s, items0, items1, dstats, n, live_dev, s_out); break;
    case 512: hipLaunchKernelGGL(k_bkt_splitters<512>, dim3(1), dim3(kBktThreads), 0, s, items0, items1, dstats, n, live_dev, s_out); break;
    case 1024: hipLaunchKernelGGL(k_bkt_splitters<1024>, dim3(1), dim3(kBktThreads), 0, s, items0, items1, dstats, n, live_dev, s_out); break;
    case 2048: hipLaunchKernelGGL(k_bkt_splitters<2048>, dim3(1), dim3(kBktThreads), 0, s, items0, items1, dstats, n, live_dev, s_out); break;
    case 4096: hipLaunchKernelGGL(k_bkt_splitters<4096>, dim3(1), dim3(kBktThreads), 0, s, items0, items1, dstats, n, live_dev, s_out); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_emit(const uint64_t* items0, const uint64_t* items1, const uint32_t* dstats, uint32_t n,
                       const uint64_t* rect, int groups, unsigned long long* wg_scratch, Stats* stats,
                       Stats* host_mapped_stats, uint32_t pair_capacity, int tiles_x, int tiles_y, void* keys,
                       bool key16, uint32_t* vals, uint2* ranges, hipStream_t s, uint32_t* fstatus) {
    hipLaunchKernelGGL(k_emit_count, dim3(groups), dim3(256), 0, s, items0, items1, dstats, n, rect, groups,
                       wg_scratch, ranges, tiles_x * tiles_y);
    hipLaunchKernelGGL(k_emit_scan, dim3(1), dim3(256), 0, s, wg_scratch, groups, pair_capacity, stats,
                       host_mapped_stats, fstatus);
    if (key16)
        hipLaunchKernelGGL(k_emit_pairs<uint16_t>, dim3(groups), dim3(256), 0, s, items0, items1, dstats, n, groups,
                           wg_scratch, pair_capacity, tiles_x, static_cast<uint16_t*>(keys), vals);
    else
        hipLaunchKernelGGL(k_emit_pairs<uint32_t>, dim3(groups), dim3(256), 0, s, items0, items1, dstats, n, groups,
                           wg_scratch, pair_capacity, tiles_x, static_cast<uint32_t*>(keys), vals);
    return hipGetLastError();
}

hipError_t launch_partition(const uint64_t* in, uint32_t n, int groups, uint32_t* counts, uint32_t* n_live,
                            uint64_t* out, const uint32_t* rect, uint32_t* pay0, uint32_t* pay1, hipStream_t s) {
    if (groups < 1 || groups > kMaxSortGroups) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_part_count, dim3(groups), dim3(256), 0, s, in, n, groups, counts);
    hipLaunchKernelGGL(k_part_scan, dim3(1), dim3(256), 0, s, counts, groups, n_live);
    hipLaunchKernelGGL(k_part_scatter, dim3(groups), dim3(256), 0, s, in, n, groups, counts, n_live, out, rect,
                       pay0, pay1);
    return hipGetLastError();
}

hipError_t launch_bin_rows(const uint64_t* items0, const uint64_t* items1, const uint32_t* dstats, uint32_t n,
                           const uint32_t* pay0, const uint32_t* pay1, int groups, uint32_t* hist,
                           uint32_t* row_items,
                           unsigned long long* row_pairs, uint32_t pair_capacity, int tiles_y, uint64_t* rows_buf,
                           int items, hipStream_t s, const uint16_t* spans, bool rank_atomic, uint32_t base,
                           uint32_t* gate, int gate_mode, const uint32_t* cut, const RowSplit* rs,
                           const uint32_t* cstart) {
    const int cut_mode = rs ? rs->cut_mode : 0;
    if (tiles_y < 1 || tiles_y > 256 || groups < 1 || groups > kMaxSortGroups / 2 ||
        (items != 4 && items != 8 && items != 16) || (gate_mode != 0 && !gate) || gate_mode < 0 || gate_mode > 2 ||
        (cut_mode != 0 && !cut) || cut_mode < 0 || cut_mode > 2)
        return hipErrorInvalidValue;
    const uint32_t* g = gate_mode == 2 ? gate : nullptr;
    const uint32_t* cut_n = rs ? rs->cut_n : nullptr;
    if (cstart && (cut_mode != 0 || gate_mode != 0 || base != 0)) return hipErrorInvalidValue;
    if (!cstart)   // with bucket chunks the bucket sort's local kernel wrote the counts
        hipLaunchKernelGGL(k_bin_rows_count, dim3(groups), dim3(256), 0, s, n, pay0, pay1, dstats, groups, tiles_y,
                           hist, base, g, cut, cut_mode, cut_n);
    hipLaunchKernelGGL(k_bin_rows_scan, dim3(256), dim3(256), 0, s, hist, groups, tiles_y, row_items, row_pairs,
                       gate, gate_mode);
    auto scatter = with_bool(rank_atomic, [&](auto ra) {
        constexpr bool RA = decltype(ra)::value;
        return tiles_y <= 128 ? (items == 4 ? k_bin_rows_scatter<4, 7, RA> : items == 8 ? k_bin_rows_scatter<8, 7, RA>
                                                                                     : k_bin_rows_scatter<16, 7, RA>)
                              : (items == 4 ? k_bin_rows_scatter<4, 8, RA> : items == 8 ? k_bin_rows_scatter<8, 8, RA>
                                                                                     : k_bin_rows_scatter<16, 8, RA>);
    });
    hipLaunchKernelGGL(scatter, dim3(groups), dim3(256), 0, s, items0, items1, dstats, pay0, pay1, n, groups, hist,
                       row_items, row_pairs, pair_capacity, tiles_y, rows_buf, spans, base, g, cut, cut_mode, cut_n,
                       cstart);
    return hipGetLastError();
}

hipError_t launch_bin_cols(const uint64_t* rows_buf, const uint32_t* row_items, const unsigned long long* row_pairs,
                           uint32_t* cbins, int col_groups, uint32_t pair_capacity, int tiles_x, int tiles_y,
                           uint32_t* vals, uint2* ranges, Stats* stats, Stats* host_mapped_stats, int items,
                           hipStream_t s, const uint32_t* dstats, int passes_launched, bool rank_atomic,
                           const uint32_t* gate, uint32_t* fstatus, int chunk) {
    if (tiles_x < 1 || tiles_x > 256 || tiles_y < 1 || tiles_y > 256 || col_groups < 1 ||
        (items != 4 && items != 8 && items != 16) || (chunk != (int)kColChunkMin && chunk != (int)kColChunkMax))
        return hipErrorInvalidValue;
    auto run = [&](auto ch) {
        constexpr uint32_t CH = decltype(ch)::value;
        hipLaunchKernelGGL(k_bin_cols_count<CH>, dim3(col_groups), dim3(256), 0, s, rows_buf, row_items, row_pairs,
                           pair_capacity, tiles_x, cbins, gate);
        hipLaunchKernelGGL(k_bin_cols_scan<CH>, dim3(tiles_y), dim3(256), 0, s, row_items, row_pairs, pair_capacity,
                           tiles_x, cbins, ranges, stats, host_mapped_stats, dstats, passes_launched, gate, fstatus);
        auto scatter = with_bool(rank_atomic, [&](auto ra) {
            constexpr bool RA = decltype(ra)::value;
            return tiles_x <= 128
                       ? (items == 4   ? k_bin_cols_scatter<4, 7, RA, CH>
                          : items == 8 ? k_bin_cols_scatter<8, 7, RA, CH>
                                       : k_bin_cols_scatter<16, 7, RA, CH>)
                       : (items == 4   ? k_bin_cols_scatter<4, 8, RA, CH>
                          : items == 8 ? k_bin_cols_scatter<8, 8, RA, CH>
                                       : k_bin_cols_scatter<16, 8, RA, CH>);
        });
        hipLaunchKernelGGL(scatter, dim3(col_groups), dim3(256), 0, s, rows_buf, row_items, row_pairs, pair_capacity,
                           tiles_x, cbins, ranges, vals, gate);
    };
    if (chunk == (int)kColChunkMin)
        run(std::integral_constant<uint32_t, kColChunkMin>{});
    else
        run(std::integral_constant<uint32_t, kColChunkMax>{});
    return hipGetLastError();
}

// cbins rows for either chunk size: a row's chunks <= its items / chunk + 1, and every row
// item holds at least one pair
uint32_t bin_col_chunks_max(uint32_t pair_capacity, int tiles_y) {
    return pair_capacity / kColChunkMin + (uint32_t)tiles_y + 1u;
}

template <typename K, int ITEMS>
static void kv_pass(const K* kin, const uint32_t* vin, K* kout, uint32_t* vout, const uint32_t* n_dev, int shift,
                    int bits, int groups, uint32_t* hist, uint32_t* totals, uint2* ranges, hipStream_t s) {
    const uint32_t mask = (1u << bits) - 1u;
    hipLaunchKernelGGL((k_kv_upsweep<K, ITEMS>), dim3(groups), dim3(kSortThreads), 0, s, kin, n_dev, shift, mask,
                       groups, hist);
    hipLaunchKernelGGL(k_radix_scan, dim3(256), dim3(256), 0, s, hist, groups, totals,
                       static_cast<const uint32_t*>(nullptr), 0, static_cast<const uint32_t*>(nullptr));
    hipLaunchKernelGGL((k_kv_downsweep<K, ITEMS>), dim3(groups), dim3(kSortThreads), 0, s, kin, vin, kout, vout,
                       n_dev, shift, bits, groups, hist, totals, ranges);
}

hipError_t launch_kv_pass(const void* keys_in, const uint32_t* vals_in, void* keys_out, uint32_t* vals_out,
                          bool key16, const uint32_t* n_dev, int shift, int bits, int groups, int items,
                          uint32_t* hist, uint32_t* totals, uint2* ranges, hipStream_t s) {
    using u16 = uint16_t;
    using u32 = uint32_t;
    const auto* k16 = static_cast<const u16*>(keys_in);
    const auto* k32 = static_cast<const u32*>(keys_in);
    auto* o16 = static_cast<u16*>(keys_out);
    auto* o32 = static_cast<u32*>(keys_out);
    if (key16 && items == 8)
        kv_pass<u16, 8>(k16, vals_in, o16, vals_out, n_dev, shift, bits, groups, hist, totals, ranges, s);
    else if (key16)
        kv_pass<u16, 16>(k16, vals_in, o16, vals_out, n_dev, shift, bits, groups, hist, totals, ranges, s);
    else if (items == 8)
        kv_pass<u32, 8>(k32, vals_in, o32, vals_out, n_dev, shift, bits, groups, hist, totals, ranges, s);
    else
        kv_pass<u32, 16>(k32, vals_in, o32, vals_out, n_dev, shift, bits, groups, hist, totals, ranges, s);
    return hipGetLastError();
}

hipError_t launch_split_sat(const uint8_t* bflag, int tiles_x, int tiles_y, uint32_t* sat, const uint32_t* gate,
                            hipStream_t s) {
    if (tiles_x < 1 || tiles_x > 256 || tiles_y < 1 || tiles_y > 256 || !gate) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_split_sat, dim3(1), dim3(256), 0, s, bflag, tiles_x, tiles_y, sat, gate);
    return hipGetLastError();
}

hipError_t launch_items_from_keys(const int* keys, uint32_t n, uint64_t* items, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_items_from_keys, dim3((n + 255) / 256), dim3(256), 0, s, keys, n, items);
    return hipGetLastError();
}

hipError_t launch_keys_from_items(const uint64_t* items, uint32_t n, int* keys, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_keys_from_items, dim3((n + 255) / 256), dim3(256), 0, s, items, n, keys);
    return hipGetLastError();
}

hipError_t launch_items_from_lwg(const gsr_lwg* rec, const uint64_t* src_perm, uint32_t n, int shift,
                                 uint32_t mask, uint64_t* items, hipStream_t s) {
    if (n)
        hipLaunchKernelGGL(k_items_from_lwg, dim3((n + 255) / 256), dim3(256), 0, s, rec, src_perm, n, shift, mask,
                           items);
    return hipGetLastError();
}

hipError_t launch_gather_lwg(const gsr_lwg* in, const uint64_t* stage1, const uint64_t* stage2, uint32_t n,
                             gsr_lwg* out, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_gather_lwg, dim3((n + 255) / 256), dim3(256), 0, s, in, stage1, stage2, n, out);
    return hipGetLastError();
}

hipError_t launch_xs_probe(const float* op, int n, float* out, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_xs_probe, dim3(grid_for(n, 256)), dim3(256), 0, s, op, n, out);
    return hipGetLastError();
}

}  // namespace gsr

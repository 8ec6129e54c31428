// gsr_kernels.hip — gfx950 (CDNA4) kernels of the 3DGS rasterizer's geometry stages (pipeline
// overview, kernel by kernel: DESIGN.md section 9).  Sections: AoS -> SoA, preprocess, blend
// cull words (the per-record half of the blend's cull), radix sort, emission, tile binning
// (with the depth split's k_split_sat), live partition, standalone sort ABI helpers (and
// k_xs_probe), launchers.  The bucket depth sort: gsr_bucket_sort.hip; what the two share (the
// tile-rectangle format, bin_rank_tile): gsr_geom_device.h.  The blend stage: gsr_blend.hip and
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
#include "gsr_geom_device.h"
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

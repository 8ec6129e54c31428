// gsr_blend_device.h — the block walk that every blend kernel shares: k_blend_w (gsr_blend.hip)
// and the passes derived from it, k_blend_aux, k_blend_contrib and k_blend_backward
// (gsr_blend_derived.hip).  One wave64 walks the tile list of one 8x8 pixel block in 64-record
// batches and must take, for every pixel and splat, the decision of render.cu:323-341: the
// derived passes add to exactly the splats the image composited only because the steps below
// exist once.  A derived pass starts with block_setup and batch_first and then, per batch,
// calls in this order: block_cull; ballot_rank and ITS OWN LDS slot stores; batch_prefetch;
// then per survivor splat_step and ITS OWN accumulation, T update and `alive` ballot.  A new
// derived pass is written against these functions, never from a copy of another kernel
// (DESIGN.md section 9).
// Inline functions only, like gsr_device.h: no kernels, no __constant__ data.
#pragma once

#include "gsr_device.h"

namespace gsr {

namespace {

// md2 cutoff of the block test from the record's xs: a lane with float md2 > -2 xs has
// -md2/2 < xs (exact scaling; the 1e-6 pad covers a subnormal -md2/2 rounding up to xs)
// and fails the alpha test.  xs = -inf: +inf (never culls); +inf: -inf (always culls).
__device__ __forceinline__ float block_cut(float xs) { return __builtin_fmaf(-2.0f, xs, 1e-6f); }

// Can any pixel of an integer rectangle reach md2 <= cut?  dx0..dy1 bound the
// (float)pixel - (float)centre offsets of the rectangle's pixels (monotone, so
// every pixel's dx lies in [dx0, dx1]).  Returns false only when the exact
// minimum of the quadratic form a dx^2 + (b+c) dx dy + e dy^2 over that
// rectangle exceeds cut by more than a bound on the float rounding of md2
// (<= ~6 ulp of |a|dx^2 + (|b|+|c|)|dx dy| + |e|dy^2, padded 10x) — so a culled
// splat could never have composited onto this block.  cut, ih and iv come from
// the record's cull word (cull_word), SMM = S M^2 with the word's S and M the largest
// |offset| of the rectangle: a conic that is not robustly positive definite has
// cut = +inf, a record without the per-record fast proof S = +inf (infinite margin);
// NaN anywhere: never culled.
__device__ __forceinline__ bool block_may_reach(float a, float b, float c, float e, float ih, float iv,
                                                float dx0, float dx1, float dy0, float dy1, float SMM, float cut) {
    // centre inside the rectangle: reachable.  Evaluated branch-free with the rest (the
    // blend's cull runs it on every lane; a branch only adds exec-mask work)
    const bool inside = (dx0 <= 0.0f) & (dx1 >= 0.0f) & (dy0 <= 0.0f) & (dy1 >= 0.0f);
    // q = a x^2 + (b + c) x y + e y^2 in Horner form with explicit fused multiply-adds
    // (5 VALU instead of 8): its rounding error stays a few ulp of the terms' magnitudes,
    // far inside the margin below (4e-6 relative)
    const float bc = b + c;
    auto q = [&](float x, float y) { return __builtin_fmaf(x, __builtin_fmaf(a, x, bc * y), (e * y) * y); };
    // The form is convex with its minimum at the splat centre (offset 0,0), which
    // lies outside the rectangle here.  A far edge never holds the rectangle's
    // minimum (from any of its points the segment toward the centre enters the
    // interior, where the form is smaller), so only the near x-edge (when 0 is not
    // in [dx0, dx1]) and the near y-edge (when 0 is not in [dy0, dy1]) are evaluated.
    const float xe = dx0 > 0.0f ? dx0 : dx1, ye = dy0 > 0.0f ? dy0 : dy1;
    // clamps as v_med3_f32: equal to fminf(fmaxf(v, lo), hi) here (lo <= hi; lo and hi
    // both NaN or neither; quiet NaN v gives lo either way), without the two
    // canonicalising v_max each fminf / fmaxf operand costs in IEEE mode
    const float qx = q(xe, __builtin_amdgcn_fmed3f(ih * xe, dy0, dy1));
    const float qy = q(__builtin_amdgcn_fmed3f(iv * ye, dx0, dx1), ye);
    const bool x_out = dx0 > 0.0f || dx1 < 0.0f, y_out = dy0 > 0.0f || dy1 < 0.0f;
    const float qm = fminf(x_out ? qx : 3.0e38f, y_out ? qy : 3.0e38f);
    const float err = __builtin_fmaf(4e-6f, SMM, 1e-3f);   // SMM = S M M (S, M: see above)
    return inside | !(qm - err > cut);
}

// 64-bit pixel mask (bit row * 8 + col) of a box descriptor built in the cull:
// bits 0-7 the column byte, 8-15 = 56 - 8 (y1 - y0), 16-23 = 8 y0.  Uniform input,
// so it compiles to scalar instructions.
__device__ __forceinline__ uint64_t box_mask(uint32_t d) {
    const uint32_t rep = (d & 0xffu) * 0x01010101u;
    const uint64_t rows = (~0ull >> ((d >> 8) & 0xffu)) << ((d >> 16) & 0xffu);
    return rows & (((uint64_t)rep << 32) | rep);
}

// The block L (tile-major index: tile << 2 | sub-block) of workgroup vb of every blend
// kernel; false for a padding workgroup.  bands > 1: band j of B consecutive blocks goes
// to XCD j mod 8; else one contiguous run of blocks per XCD (xcd_chunk).  (k_blend_w's comment.)
__device__ __forceinline__ bool blend_block_index(int vb, int ntiles, int bands, int& L) {
    if (bands > 1) {
        const int nu = 4 * ntiles;
        const int B = (nu + 8 * bands - 1) / (8 * bands);
        const int k = vb >> 3;
        L = ((k / B) * 8 + (vb & 7)) * B + k % B;
        if (L >= nu) return false;
    } else {
        if (vb >= ntiles * 4) return false;
        L = xcd_chunk(vb, ntiles * 4);
    }
    return true;
}

// What a derived pass's wave knows of its block before the walk: block L (blend_block_index)
// at pixels (bx.., by..) with the tile list idx[beg, end); lane = pixel (px, py), `inside`
// the covered area (pixels outside it start saturated, T = 0, and composite nothing).
struct BlockSetup {
    int L, bx, by;
    uint32_t beg, end;
    int lane, px, py;
    bool inside;
    float fpx, fpy;
};

// The derived passes' prologue (k_blend_w interleaves its depth-split and timeline work with
// the same steps); false for a padding workgroup.
__device__ __forceinline__ bool block_setup(BlockSetup& B, const uint2* __restrict__ ranges, int tiles_x,
                                            int tiles_y, int cover_w, int cover_h, int bands) {
    if (!blend_block_index((int)blockIdx.x, tiles_x * tiles_y, bands, B.L)) return false;
    const int tile = B.L >> 2, sub = B.L & 3;
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    B.lane = (int)(threadIdx.x & 63u);
    const uint2 rr = ranges[tile];                          // {~start, end}, zero = empty
    B.beg = rr.y ? ~rr.x : 0u;
    B.end = rr.y;
    B.bx = tx * GSR_TILE_PX + (sub & 1) * 8;
    B.by = ty * GSR_TILE_PX + (sub >> 1) * 8;
    B.px = B.bx + (B.lane & 7);
    B.py = B.by + (B.lane >> 3);
    B.inside = B.px < cover_w && B.py < cover_h;
    B.fpx = (float)B.px;
    B.fpy = (float)B.py;
    return true;
}

// One batch of the list walk: lane l holds record l of the batch's 64 — ra the conic
// {a, b, c, e}, rb {opacity, red, green, blue}, rc {cx, cy, xmin | xmax << 16, ymin |
// ymax << 16}, rd the cull word {xs, ih, iv, S} — and its Gaussian index cidx; nidx is the
// index of the lane's record in the NEXT batch, loaded one batch ahead of its record.
struct RecordBatch {
    uint4 ra, rb, rc, rd;
    uint32_t cidx, nidx;
};

// batch_first and batch_prefetch (k_blend_contrib, k_blend_backward) mirror the load and
// prefetch that blend_block (gsr_blend.hip) and k_blend_aux (gsr_blend_derived.hip) keep in
// plain locals, the copies to watch: a struct passed to these two functions reaches scalar
// replacement only after inlining, which at k_blend_w's 64-VGPR budget spills its fast-exp
// instantiation (12 B of scratch) and slows k_blend_aux's 4-channel one by about 1 %.

// The first batch of idx[beg, end) and the second batch's indices.
__device__ __forceinline__ void batch_first(RecordBatch& B, const uint32_t* __restrict__ idx,
                                            const uint4* __restrict__ rec, uint32_t beg, uint32_t end, int lane) {
    B.ra = make_uint4(0, 0, 0, 0);
    B.rb = B.ra;
    B.rc = B.ra;
    B.rd = B.ra;
    B.nidx = 0;
    B.cidx = 0;
    if (beg + lane < end) {
        B.cidx = idx[beg + lane];
        const uint4* R = rec + 4 * (uint64_t)B.cidx;
        B.ra = R[0];
        B.rb = R[1];
        B.rc = R[2];
        B.rd = R[3];
    }
    if (beg + 64 + lane < end) B.nidx = idx[beg + 64 + lane];
}

// Prefetch during the batch at `base`: records of batch k+1, indices of batch k+2.  A kernel
// calls it after its survivors' first LDS stores (which read the current records) and
// before anything that waits on memory; whatever it still needs of the current batch
// afterwards it saves in registers first.
__device__ __forceinline__ void batch_prefetch(RecordBatch& B, const uint32_t* __restrict__ idx,
                                               const uint4* __restrict__ rec, uint32_t base, uint32_t end, int lane) {
    if (base + 64 + lane < end) {
        B.cidx = B.nidx;
        const uint4* R = rec + 4 * (uint64_t)B.nidx;
        B.ra = R[0];
        B.rb = R[1];
        B.rc = R[2];
        B.rd = R[3];
    }
    if (base + 128 + lane < end) B.nidx = idx[base + 128 + lane];
}

// The cull of one batch against the block (bx, by), lane = record: the AABB against the
// block, the live-pixel filter and the exact ellipse-vs-block test (block_may_reach).
// Returns whether the record survives (some live pixel of the block may composite it), and
//   dsc  its box as a descriptor (box_mask), expanded on the scalar unit by the compositing loop
//   SMM  S M^2, the per-block part of the fast-path proof (coef_ok; k_blend_w alone reads it)
// cnt: records in the batch.  live_b: the pixels not yet saturated at the batch start; T only
// decreases, so a record whose in-box pixels are all saturated here can never be taken in
// this batch.
// Branch-free over the 64 lanes: nearly every batch has lanes on both sides of each test, so
// branches would only add exec-mask work (lanes >= cnt hold stale registers: their results
// are discarded through `valid`).
struct BlockCull {
    uint32_t dsc;
    float SMM;
};
__device__ __forceinline__ bool block_cull(BlockCull& r, const uint4& ra, const uint4& rc, const uint4& rd, int bx,
                                           int by, int lane, uint32_t cnt, uint64_t live_b) {
    const bool valid = (uint32_t)lane < cnt;
    const int xmin = (int)(rc.z & 0xffffu), xmax = (int)(rc.z >> 16);
    const int ymin = (int)(rc.w & 0xffffu), ymax = (int)(rc.w >> 16);
    const bool box_hit = valid & !((xmax < bx) | (xmin > bx + 7) | (ymax < by) | (ymin > by + 7));
    const float cx = __uint_as_float(rc.x), cy = __uint_as_float(rc.y);
    const float a = __uint_as_float(ra.x), b = __uint_as_float(ra.y);
    const float c = __uint_as_float(ra.z), e = __uint_as_float(ra.w);
    const int x0 = max(xmin - bx, 0), x1 = min(xmax - bx, 7);
    const int y0 = max(ymin - by, 0), y1 = min(ymax - by, 7);
    const float dx0 = (float)(bx + x0) - cx, dx1 = (float)(bx + x1) - cx;
    const float dy0 = (float)(by + y0) - cy, dy1 = (float)(by + y1) - cy;
    // the box as a descriptor (box_mask: bit row * 8 + col of the block = pixel inside the
    // AABB): column byte | (56 - 8 (y1 - y0)) << 8 | 8 y0 << 16
    // (shift counts masked to the hardware's: only lanes outside the box can have them out
    // of range, and their results are discarded)
    const uint32_t colb = (0xffu >> ((uint32_t)(7 - (x1 - x0)) & 31u)) << ((uint32_t)x0 & 31u);
    const uint32_t rsh = (uint32_t)(56 - 8 * (y1 - y0)) & 63u, lsh = (uint32_t)(8 * y0) & 63u;
    r.dsc = colb | (rsh << 8) | (lsh << 16);
    // the same 64-bit mask here, only for the saturation filter below
    const uint64_t rows = (~0ull >> rsh) << lsh;
    const uint32_t rep = __builtin_amdgcn_perm(colb, colb, 0u);   // colb in every byte
    const uint64_t lrows = rows & live_b;
    // cull word (cull_word): per-record parts of the block test and the proof
    const float S = __uint_as_float(rd.w);
    const float M = fmaxf(fmaxf(fabsf(dx0), fabsf(dx1)), fmaxf(fabsf(dy0), fabsf(dy1)));
    r.SMM = S * M * M;
    return box_hit & ((((uint32_t)lrows | (uint32_t)(lrows >> 32)) & rep) != 0u) &
           block_may_reach(a, b, c, e, __uint_as_float(rd.y), __uint_as_float(rd.z), dx0, dx1, dy0, dy1, r.SMM,
                           block_cut(__uint_as_float(rd.x)));
}

// A survivor's rank in list order: the set bits of the hit ballot m below this lane.
__device__ __forceinline__ uint32_t ballot_rank(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// The exact one-splat step (render.cu:329-335 with gsr_blend_md2, gsr_blend_expf and plain
// selects) of the pixel (fpx, fpy) with transmittance T against one survivor — centre, conic,
// opacity and `box`, its box_mask: returns the decision `take` of render.cu:323-341, with the
// alpha it composites with.  dx, dy, ee and oe (opacity * ee, alpha before the 0.99 clamp) are for
// k_blend_backward; unused, they drop out after inlining.  The caller updates T (render.cu:339,
// T * (1.0f - alpha) where `take`) and its `alive` ballot where it needs them.
struct SplatStep {
    float dx, dy, ee, oe, alpha;
};
__device__ __forceinline__ bool splat_step(SplatStep& s, float fpx, float fpy, float cx, float cy, float a, float b,
                                           float c, float e, float opacity, uint64_t box, float T) {
    s.dx = fpx - cx;
    s.dy = fpy - cy;
    const float md = gsr_blend_md2(s.dx, s.dy, a, b, c, e);
    s.ee = gsr_blend_expf(-0.5f * md);
    s.oe = opacity * s.ee;
    s.alpha = fminf(s.oe, 0.99f);
    const bool in = __builtin_amdgcn_inverse_ballot_w64(box);
    return in & !(T < 1e-3f) & !(s.alpha < 1e-3f);
}

// The grid of every blend kernel (blend_block_index): `bands` bands of band_tiles tiles per XCD,
// dealt round-robin; ng is padded to whole rounds.  Too small for two rounds: one run per XCD
// (bands 1).  Host code.
inline void blend_grid(int nt, int band_tiles, int& bands, int& ng) {
    bands = 1;
    ng = 4 * nt;
    if (band_tiles > 0 && (nt + 8 * band_tiles - 1) / (8 * band_tiles) > 1) {
        bands = (nt + 8 * band_tiles - 1) / (8 * band_tiles);
        ng = 8 * bands * ((4 * nt + 8 * bands - 1) / (8 * bands));
    }
}

}  // namespace

}  // namespace gsr

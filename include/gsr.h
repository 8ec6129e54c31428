/*
 * gsr.h — C ABI of the MI355X-native 3D Gaussian splatting rasterizer.
 *
 * Two groups of entry points:
 *
 *  1. DROP-IN BOUNDARY — the exact symbols the reference viewer links
 *     against.  A viewer built against the reference's
 *     render.cuh / misc.cuh links against libgsr.so unchanged:
 *
 *       preprocessCUDAGaussians   replaces render.cu:871-1157 (decl render.cuh:27-37)
 *       loadGaussianCudaFromPly   replaces misc.cu:13-134     (decl misc.cuh:4, C++ linkage)
 *       oneSweep3DGaussianSort    replaces render.cu:194-264  (decl render.cuh:8-11)
 *       oneSweepSort              replaces onesweep.cu:190-250 (decl onesweep.cuh:8)
 *
 *  2. NATIVE API (gsr_*) — stream-ordered, device-resident, no per-frame
 *     allocation: a persistent context (workspace sized by high-water mark),
 *     the three pipeline stages the reference names "Preprocess + Sort +
 *     Render" as separate calls, readback hooks used by the parity tests, and
 *     the host-side camera / PLY helpers that mirror the reference's
 *     camera.cpp and gaussians.cpp so tests and benches can build inputs
 *     exactly like the viewer does.
 *
 * Errors: every int-returning function returns 0 on success and a negative
 * GSR_E* code on failure; gsr_last_error() returns the message.  The void
 * drop-in functions keep the reference's behaviour (print the error to
 * stderr and return, render.cu:914-923).
 */
#ifndef GSR_H
#define GSR_H

#include <stddef.h>
#include <stdint.h>
#include "gsr_types.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    GSR_OK = 0,
    GSR_E_ARG = -1,        /* invalid argument */
    GSR_E_HIP = -2,        /* HIP runtime error (no device, OOM, launch failure) */
    GSR_E_IO = -3,         /* file missing / unreadable / truncated */
    GSR_E_FORMAT = -4,     /* unsupported PLY format */
    GSR_E_OVERFLOW = -5,   /* an earlier frame is incomplete and must be re-rendered: its pairs
                              overflowed the pair buffer (grown now), its depth sort needed more
                              digit passes than the adaptive pass budget launched (budget reset to
                              four), or it was a speculative depth-split frame (GSR_TUNE_DEPTH_SPLIT,
                              no phase B queued) whose phase A left an 8x8 block unsaturated
                              (speculation stopped).  Any of these can happen at any frame, not only
                              during warm-up; gsr_render_path_status names the frames.  The
                              code can arrive on a later call than the frame it refers to: every
                              frame rendered since the last call that returned GSR_OK (or since the
                              last gsr_sync) must be re-rendered. */
    GSR_E_DISPLAY = -6     /* display interop: no current GL context / GL registration failed (gsr_gl.h) */
};

/* Scene layout accepted by the render entry points. */
enum {
    GSR_LAYOUT_SCENE_BLOCK = 0,   /* our SoA block (gsr_scene_header + arrays) */
    GSR_LAYOUT_AOS = 1,           /* reference Gaussian[] (240 B records) */
    GSR_LAYOUT_SCENE_BLOCK_4D = 2, /* 4D SoA block (GSR_SCENE4D_NARRAYS), rendered at gsr_set_time() */
    GSR_LAYOUT_SCENE_BLOCK_SH3 = 3 /* SH-3 block (GSR_SCENE_SH3_NARRAYS): degree-3 colour, clamped at 0 */
};

/* PLY loading flags (gsr_ply_read_host_ex / gsr_load_ply_device_ex). */
enum {
    GSR_PLY_TYPED = 1,  /* hardened reader: declared property types, ascii and big-endian
                           formats, other elements skipped, "nx" accepted.
                           Off = the reference's reader exactly (every property a 4-B float). */
    GSR_PLY_SH3 = 2     /* "Inria-correct" SH: all 45 f_rest, channel-major, into a 59-array
                           block rendered with degree-3 SH (off = the reference's 24 f_rest) */
};

/* Stage indices for gsr_stage_times(). */
enum {
    GSR_STAGE_PREPROCESS = 0,     /* cull + SH colour + projection + covariance + AABB */
    GSR_STAGE_DEPTH_SORT = 1,     /* stable radix sort of (depth, index) */
    GSR_STAGE_EMIT = 2,           /* pair emission, or the binning row pass */
    GSR_STAGE_TILE_SORT = 3,      /* stable radix sort of pairs by tile, or the binning column pass */
    GSR_STAGE_RANGES = 4,         /* per-tile [start, end) from sorted pairs */
    GSR_STAGE_BLEND = 5,          /* front-to-back alpha compositing (with the depth split: phase A's) */
    GSR_STAGE_RESUME = 6,         /* depth split phase B: binning the rest of the depth order and
                                     resuming the blocks phase A left unsaturated (0 on other frames) */
    GSR_NUM_STAGES = 7
};

#define GSR_TILE_PX 16            /* internal tile edge (pixels); output is tile-invariant */
#define GSR_SPLAT_RECORD_BYTES 64 /* per-Gaussian splat record written by preprocess */

/* ---------------------------------------------------------------- drop-in */

/* render.cu:871-881.  d_gaussians: a device scene block from
 * loadGaussianCudaFromPly (our SoA layout) OR a device Gaussian[] array in
 * the reference's AoS layout (detected by the header magic).  out_pixels:
 * HOST buffer of 3*tile_W*tile_H floats, planar RGB, row 0 = bottom (NDC -1).
 * tile_W/tile_H are the image size; the num_tile / stride arguments follow
 * TilingInformation (gaussians.hpp:47-58) and only bound which pixels are
 * covered (pixels at x >= num_tile_x*width_stride or y >= num_tile_y*
 * height_stride stay 0 as in renderGaussians, render.cu:285-363).
 * Synchronous; uses a process-wide context guarded by a mutex. */
void preprocessCUDAGaussians(gsr_gaussian* d_gaussians, float* out_pixels, int num_gaussians,
                             gsr_camera cam, int num_tile_y, int num_tile_x, int width_stride,
                             int height_stride, int tile_W, int tile_H, float k);

/* C twin of loadGaussianCudaFromPly (misc.cu:13-134) for FFI callers:
 * returns a device scene block (free with hipFree or gsr_scene_free), or
 * NULL on failure; *out_numGaussians is set once the header is parsed. */
gsr_gaussian* gsr_load_ply_device(const char* filename, int* out_numGaussians);
/* Same with loader flags (GSR_PLY_TYPED | GSR_PLY_SH3).  If out_narrays is
 * non-NULL, a file carrying the 4D properties (trbf_center, trbf_scale,
 * motion_0..8) loads as a 4D scene block (*out_narrays = 49); GSR_PLY_SH3
 * gives an SH-3 block (59); else 38. */
gsr_gaussian* gsr_load_ply_device_ex(const char* filename, int* out_numGaussians, int flags, int* out_narrays);

/* render.cu:194-264: stable sort of N host-side lightWeightGaussian records
 * by the low num_bits bits of radix_id, in place; *kernel_ms = device time. */
void oneSweep3DGaussianSort(gsr_lwg* d_in, int N, int num_bits, float* kernel_ms);

/* onesweep.cu:190-250: sort N host ints (keys in [0, maxVal], non-negative)
 * ascending into output; *kernel_ms = device time of the sort passes. */
void oneSweepSort(int* input, int* output, int N, int maxVal, float* kernel_ms);

/* ---------------------------------------------------------------- context */

typedef struct gsr_context gsr_context;

gsr_context* gsr_create(void);
void gsr_destroy(gsr_context* ctx);

/* Pre-size the workspace for n Gaussians and `pairs` (tile, Gaussian) pairs. */
int gsr_reserve(gsr_context* ctx, int64_t n, int64_t pairs);

/* Whole frame, stream-ordered (stream = hipStream_t or NULL for the default
 * stream).  d_out: DEVICE buffer of 3*W*H floats (planar, row 0 = bottom).
 * Reference tiling arguments as in preprocessCUDAGaussians; pass
 * num_tile_x = num_tile_y = 1 and strides = W, H for "cover the image".
 * Returns GSR_E_OVERFLOW if an earlier frame was incomplete (pair buffer
 * overflow, grown; a depth sort short of passes, budget reset; or a speculative
 * depth-split frame that needed phase B): re-render every frame since the last
 * clean return, see GSR_E_OVERFLOW. */
int gsr_render(gsr_context* ctx, const void* d_scene, int layout, int64_t n,
               const gsr_camera* cam, int W, int H, int num_tile_x, int num_tile_y,
               int width_stride, int height_stride, float k, float* d_out, void* stream);

/* Auxiliary render targets: gsr_render's frame with, besides (or instead of) the image,
 * the accumulated alpha, the depth and up to GSR_AUX_MAX_FEATURES composited per-Gaussian
 * feature channels.  The three-channel gsr_render path does not carry them: this entry
 * point runs its own blend kernel over the same tile lists.
 *
 * For a pixel that composites splats i1, i2, ... (the decisions of render.cu:323-341), with
 * T_j the transmittance before splat j and alpha_j its clamped alpha, every channel
 * accumulates like a colour channel, acc = fma(v * alpha_j, T_j, acc) in list order, with
 *   v = 1.0f                  alpha: the coverage sum alpha_j T_j = 1 - final T (rounded
 *                             its own way), in [0, 1]; over a background B the composite is
 *                             image + (1 - alpha) * B
 *   v = -Z                    depth: Z is the splat's view-space z, the float behind its
 *                             depth key (key = -Z * 1e6 saturated), so -Z is its positive
 *                             distance along the view axis
 *   v = d_features[f*n + i]   feature f of Gaussian i
 * Depth (and the features) are the UN-NORMALISED sums: the expected depth of what the pixel
 * composited is depth / alpha where alpha > 0, and the caller divides.
 * d_out (may be NULL) receives the image gsr_render produces with the exact blend
 * (GSR_TUNE_BLEND_EXP 0), bit for bit, whatever that knob is set to.
 * All planes are W*H floats, planar, row 0 = bottom; pixels outside the covered area (the
 * num_tile / stride arguments) and pixels no splat reaches are 0 in every plane.
 *
 * An aux frame always runs the exact blend in one phase: the depth split does not apply
 * and its controller (split point, speculation, retry counters) is left exactly as it
 * was.  Sorting, binning, overflow reporting (GSR_E_OVERFLOW, gsr_sync), the scene layouts
 * (4D scenes render at gsr_set_time) and timing are gsr_render's; the aux blend is timed
 * under GSR_STAGE_BLEND.  Aux frames write no diagnostics: the blend counters, the take
 * map and the stamps keep the last non-aux frame's values.  Stream-ordered; allocates
 * only when a high-water mark grows (workspace: n floats for the depth channel, 32 n bytes
 * for more than four features).
 * GSR_E_ARG, before any device work: every output NULL, nfeat outside
 * [0, GSR_AUX_MAX_FEATURES], nfeat > 0 without d_features or d_feat_out, or aux NULL. */
#define GSR_AUX_MAX_FEATURES 8
typedef struct gsr_aux_targets {
    float*       d_alpha;     /* W*H floats, or NULL */
    float*       d_depth;     /* W*H floats, or NULL */
    const float* d_features;  /* nfeat arrays of n floats, planar (feature f of Gaussian i at [f*n + i]);
                                 NULL iff nfeat == 0 */
    int          nfeat;       /* 0..GSR_AUX_MAX_FEATURES */
    float*       d_feat_out;  /* nfeat*W*H floats planar; required iff nfeat > 0 */
} gsr_aux_targets;
int gsr_render_aux(gsr_context* ctx, const void* d_scene, int layout, int64_t n, const gsr_camera* cam,
                   int W, int H, int num_tile_x, int num_tile_y, int width_stride, int height_stride,
                   float k, float* d_out, const gsr_aux_targets* aux, void* stream);

/* Contribution statistics: which Gaussians made gsr_render's image of this frame, and how
 * much each contributed (picking, pruning and level of detail, visibility sets).  No image
 * is written: this entry point runs its own blend kernel over the same tile lists.
 *
 * Pixel p composites splat i when it takes it under the exact blend's decisions (the
 * reference's, render.cu:323-341: inside the splat's box, T >= 1e-3, alpha >= 1e-3).  The
 * weight of that take is w_i(p) = fma(alpha, T, 0) — one rounding of alpha * T, alpha the
 * clamped alpha and T the transmittance before the splat — so 0 < w <= 0.99, and the
 * accumulated alpha of gsr_render_aux is the sum of a pixel's weights.
 *
 *   d_count[i]   += the number of pixels that composited Gaussian i
 *   d_weight[i]  += the sum over those pixels of rint(w_i(p) * GSR_CONTRIB_WEIGHT_ONE)
 *                   (round to nearest even; fixed point, 2^24 = 1.0)
 *   d_max[i]      = max(d_max[i], float bits of the largest w_i(p)); the bits of positive
 *                   floats order as unsigned integers, 0 = never composited
 *   d_id[p]       = the composited Gaussian with the largest w_i(p): a later splat of the
 *                   list replaces the held one only when its w is strictly greater; -1 where
 *                   the pixel composited nothing or lies outside the covered area
 *                   (W*H words, row 0 = bottom, as the image)
 *
 * The three per-Gaussian arrays (n words each) ACCUMULATE and are never cleared by the
 * library: the caller zeroes them once, and every later frame (another camera, another
 * time of a 4D scene) adds to them on `stream`, so a camera path yields multi-view totals.
 * All three reductions are integer and independent of order: results are reproducible bit
 * for bit.  d_id is OVERWRITTEN by every frame.  Every pointer may be NULL; a statistic
 * that is not asked for is not computed.
 *
 * An incomplete frame adds nothing: a frame that overflows the pair buffer or the depth
 * pass budget (reported through GSR_E_OVERFLOW or gsr_sync, as for gsr_render) leaves
 * d_count, d_weight and d_max exactly as they were, and d_id unspecified; render it again.
 *
 * The frame policy is gsr_render_aux's: one phase with the exact blend whatever
 * GSR_TUNE_BLEND_EXP says, the depth split off and its controller left exactly as it was;
 * sorting, binning and the scene layouts (4D scenes render at gsr_set_time) are
 * gsr_render's; the blend is timed under GSR_STAGE_BLEND; no diagnostics are written (the
 * blend counters, the take map and the stamps keep the last non-aux frame's values).
 * Stream-ordered, no allocation of its own.  Not offered through gsr_render_path.
 * GSR_E_ARG, before any device work: every pointer NULL, or out NULL. */
#define GSR_CONTRIB_WEIGHT_ONE 16777216u          /* 2^24: fixed-point scale of d_weight */
typedef struct gsr_contrib_targets {
    uint32_t* d_count;   /* n words, accumulated, or NULL */
    uint64_t* d_weight;  /* n words, accumulated, or NULL */
    uint32_t* d_max;     /* n words, accumulated (max of float bits), or NULL */
    int32_t*  d_id;      /* W*H words, overwritten, or NULL */
} gsr_contrib_targets;
int gsr_render_contrib(gsr_context* ctx, const void* d_scene, int layout, int64_t n, const gsr_camera* cam,
                       int W, int H, int num_tile_x, int num_tile_y, int width_stride, int height_stride,
                       float k, const gsr_contrib_targets* out, void* stream);

/* Backward pass of the blend: how this frame's image and accumulated alpha react to each
 * Gaussian's SPLAT RECORD — the colour, opacity, 2D conic (inv_covar[0..3] = a, b, c, e) and
 * 2D centre (px_x, px_y) that the preprocess hands to the blend.  Carrying these on to the
 * scene's position, scale, rotation and SH arrays (the projection's backward) is not part of
 * this call: gsr_project_backward does it, gsr_render_backward_scene both.  No image is written: the call runs its own blend kernel over the tile lists.
 *
 * With upstream gradients g = (g_r, g_g, g_b) = d_grad_image and g_A = d_grad_alpha at every
 * pixel (a NULL input counts as zeros), the function differentiated is
 *   L = sum over pixels of g_rgb . image + g_A alpha
 * of the exact blend.  For pixel p and the splats j = 1, 2, ... it takes (the reference's
 * tests, render.cu:323-341: inside the box, T >= 1e-3, alpha >= 1e-3):
 *   dx = p.x - cx, dy = p.y - cy, md2 = dx (a dx + b dy) + dy (c dx + e dy),
 *   E = exp(-md2 / 2), alpha = min(o E, 0.99),
 *   image += colour alpha T, alpha_acc += alpha T, T <- T (1 - alpha).
 * The take decisions are piecewise constant and get no gradient.  With u_j = g_rgb .
 * colour_j + g_A, P_j = sum_{k <= j} u_k alpha_k T_k and G = P_last:
 *   d_color[ch]  += g_ch alpha_j T_j
 *   dL/dalpha_j   = T_j u_j - (G - P_j) / (1 - alpha_j)
 *   where o E > 0.99 the clamp is active and nothing reaches o or the geometry; otherwise
 *   d_opacity    += dL/dalpha E,        dmd = -1/2 o E dL/dalpha,
 *   d_conic      += dmd (dx^2, dx dy, dx dy, dy^2),
 *   d_center     += -dmd (2 a dx + (b + c) dy, (b + c) dx + 2 e dy).
 * The centre is differentiated as a real variable in the record's pixel coordinates, although
 * the record itself holds whole pixels; mapping it further is the projection backward's
 * business.  Pixels outside the covered area contribute nothing, whatever their g.
 *
 * The outputs are planar, element [c * n + i] for Gaussian i — the layout gsr_gather_planes
 * cuts down after a prune.  Every output ACCUMULATES and is never cleared by the library, so
 * a camera path sums a multi-view batch.  They are summed with float atomics whose order of
 * arrival is not fixed: unlike every other output of this library, the results are NOT
 * reproducible bit for bit; two runs can differ in the last bits.  An output that is not
 * asked for is not computed.  A Gaussian no pixel composited is not touched at all.
 *
 * An incomplete frame (GSR_E_OVERFLOW here or from gsr_sync) adds nothing; render it again.
 * The frame policy is gsr_render_contrib's: one phase with the exact blend whatever
 * GSR_TUNE_BLEND_EXP says, the depth split off and its controller untouched, the blend timed
 * under GSR_STAGE_BLEND, no diagnostics; sorting, binning and the scene layouts are
 * gsr_render's.  Stream-ordered, no allocation of its own.  Not offered through
 * gsr_render_path.  GSR_E_ARG, before any device work: bw NULL, both gradient inputs NULL,
 * or every output NULL. */
typedef struct gsr_backward_targets {
    const float* d_grad_image;  /* 3*W*H, planar, row 0 = bottom: dL/d image; or NULL */
    const float* d_grad_alpha;  /* W*H: dL/d (gsr_render_aux's accumulated alpha); or NULL */
    float* d_color;    /* 3 planes of n floats: dL/d record colour     (ACCUMULATED), or NULL */
    float* d_opacity;  /* n floats:             dL/d record opacity    (ACCUMULATED), or NULL */
    float* d_conic;    /* 4 planes of n floats: dL/d inv_covar[0..3]   (ACCUMULATED), or NULL */
    float* d_center;   /* 2 planes of n floats: dL/d (px_x, px_y)      (ACCUMULATED), or NULL */
} gsr_backward_targets;
int gsr_render_backward(gsr_context* ctx, const void* d_scene, int layout, int64_t n, const gsr_camera* cam,
                        int W, int H, int num_tile_x, int num_tile_y, int width_stride, int height_stride,
                        float k, const gsr_backward_targets* bw, void* stream);

/* Backward pass of the projection: carries gsr_render_backward's record gradients on to the
 * scene arrays a .ply stores — position, opacity, scale, rotation, SH, and the temporal arrays
 * of a 4D block.  With it the chain render -> gsr_render_backward -> gsr_project_backward gives
 * dL/d scene for fine-tuning, or re-fitting after a prune (gsr_gather_planes cuts the planes).
 *
 * The function differentiated is the preprocess's map from Gaussian i's scene arrays to its
 * splat record, taken as a real-valued function:
 *   p       the stored position; for a 4D block the position at gsr_set_time's t, dt = t -
 *           trbf_center, p = x + m0 dt + m3 dt^2 + m6 dt^3 (y, z with m1/m4/m7, m2/m5/m8)
 *   v       = V [p, 1] = (X, Y, Z, .), clip = P v, ndc = clip.xyz / clip.w; V and P are taken
 *           as general row-major 4x4 matrices
 *   centre  = ((ndc_x + 1) W/2, (ndc_y + 1) H/2); the record holds round() of it, and the
 *           rounding is differentiated as the identity (straight-through): the contract
 *           gsr_render_backward states for its d_center
 *   Sigma   = (R S)(R S)^T, R from the normalised quaternion, S = diag(scale); Sigma_c = Rc
 *           Sigma Rc^T with the camera's r_cam
 *   J       = [[fx/Z, 0, -fx X/Z^2], [0, fy/Z, -fy Y/Z^2]], fx, fy of gsr_camera_intrinsics
 *   M       = D o (J Sigma_c J^T), D the pixel factors (W/2)^2, (W/2)(H/2), (H/2)(W/2), (H/2)^2
 *   conic   (a, b, c, e) = (M11, -M01, -M10, M00) / det M, that is [[a, b], [c, e]] = M^-1; b
 *           and c are separate record fields with separate gradients (not symmetrised)
 *   colour  dir = (p - camera position) / |.| (zero when the norm is <= 1e-8); SH bands 0..2
 *           plus 0.5, clamped to [0, 1] — an SH-3 block: bands 0..3, clamped at 0 only; the
 *           clamp passes gradient only where the unclamped value lies strictly inside; the
 *           colour's dependence on the position through dir is part of d_position
 *   opacity the stored value; for a 4D block times exp(-(dt / trbf_scale)^2), with gradients
 *           to the opacity, trbf_center, trbf_scale and, through p, the nine motion arrays
 * The extent, the pixel box, the tile rects, the depth key, k, every cull decision and the
 * camera get no gradient.  The gradients are with respect to the STORED values (the activated
 * opacity and scales of the scene block): a caller that optimises raw .ply values multiplies
 * by op (1 - op) and by the scale itself.
 *
 * Inputs (gsr_record_grads) are gsr_render_backward's outputs, planar [c * n + i]; a NULL
 * plane group counts as zeros.  Outputs (gsr_scene_grads), planar [c * n + i] in the array
 * order of the scene block, ACCUMULATE and are never cleared by the library; an output that is
 * not asked for is not computed.
 *
 * A Gaussian takes part when its record is defined and its upstream is not all zero:
 *   - skipped, on the preprocess's own float32 comparisons: non-finite view position or ndc,
 *     Z >= -nearClip, ndc z outside [-1, 1], det M non-finite or < 1e-8;
 *   - skipped, before its scene arrays are loaded: all ten upstream entries +-0.
 * A skipped Gaussian is not touched at all.  The screen-extent reject and the 4D temporal cull
 * are not evaluated again: what they drop never composites and arrives with zero upstream.
 *
 * One thread owns one Gaussian and adds to each plane with a plain load, add and store, no
 * atomics: for given inputs the results ARE reproducible bit for bit (unlike
 * gsr_render_backward's).  Stream-ordered: no allocation, no synchronisation.  The context
 * gives the lock and the 4D time only; its records, tile lists, depth-split controller, timing
 * and diagnostics stay exactly as they were, and a readback after this call still refers to
 * the last rendered frame.  Not offered through gsr_render_path.
 * GSR_E_ARG, before any device work: ctx, in or out NULL; every input NULL or every output
 * NULL; GSR_LAYOUT_AOS (gradient planes of an AoS array have no consumer here); d_temporal on
 * a block that is not 4D; the frame arguments gsr_render refuses (camera, image size, n,
 * scene, layout). */
typedef struct gsr_record_grads {      /* inputs: gsr_render_backward's outputs, planar [c*n + i]; NULL = zeros */
    const float* d_color;    /* 3 planes */
    const float* d_opacity;  /* 1 */
    const float* d_conic;    /* 4: a, b, c, e */
    const float* d_center;   /* 2 */
} gsr_record_grads;
typedef struct gsr_scene_grads {       /* outputs, planar [c*n + i], ACCUMULATED, NULL = not computed */
    float* d_position;  /* 3 planes: arrays 0..2 */
    float* d_opacity;   /* 1: array 3 (the stored, activated value) */
    float* d_scale;     /* 3: arrays 4..6 (stored, activated) */
    float* d_rot;       /* 4: arrays 7..10 (raw w,x,y,z, through the normalisation) */
    float* d_sh;        /* 27 planes (48 for an SH-3 block), array order of the block */
    float* d_temporal;  /* 11 planes: trbf_center, trbf_scale (stored), motion_0..8; 4D blocks only */
} gsr_scene_grads;
int gsr_project_backward(gsr_context* ctx, const void* d_scene, int layout, int64_t n, const gsr_camera* cam,
                         int W, int H, float k, const gsr_record_grads* in, const gsr_scene_grads* out, void* stream);

/* The whole backward of one frame in one call: gsr_render_backward's frame into ten
 * record-gradient planes, then gsr_project_backward from them into `out`.
 * The planes (colour 3, opacity 1, conic 4, centre 2, each n floats, in this order) sit in
 * d_record_scratch, or, when that is NULL, in a workspace of the context (10 n floats, grown
 * by high-water mark: the only allocation).  The call zeroes them on `stream` first; a
 * caller's scratch holds the frame's record gradients afterwards (the densification criterion
 * reads its centre planes).
 * Frame policy, GSR_E_OVERFLOW reporting and gsr_sync are gsr_render_backward's.  An
 * incomplete frame adds nothing to `out`: its blend adds nothing, the planes stay zero and
 * every Gaussian is skipped; render it again.  The blend's atomics make the planes, and with
 * them `out`, differ in the last bits from run to run; for given planes the projection is
 * reproducible.  GSR_E_ARG, before any device work: ctx or out NULL, both gradient inputs
 * NULL, every output NULL, GSR_LAYOUT_AOS, d_temporal on a block that is not 4D, the frame
 * arguments gsr_render refuses. */
int gsr_render_backward_scene(gsr_context* ctx, const void* d_scene, int layout, int64_t n, const gsr_camera* cam,
                              int W, int H, int num_tile_x, int num_tile_y, int width_stride, int height_stride, float k,
                              const float* d_grad_image, const float* d_grad_alpha,
                              float* d_record_scratch /* 10 planes of n floats, or NULL */,
                              const gsr_scene_grads* out, void* stream);

/* The backward pass with gsr_render_aux's depth and feature planes: gsr_render_backward,
 * gsr_project_backward and gsr_render_backward_scene with two more kinds of upstream
 * gradient, so a loss may read every plane the renderer composites.
 *
 * gsr_render_backward_aux.  With g_D = d_grad_depth (the gradient of gsr_render_aux's d_depth,
 * the UN-NORMALISED sum of -Z alpha T) and g_f = plane f of d_grad_feat (the gradient of
 * d_feat_out plane f), W*H planes like the others, a NULL plane counting as zeros, the
 * function differentiated is
 *   L = sum over pixels of g_rgb . image + g_A alpha + g_D depth + sum_f g_f feat_f
 * of the exact blend, with gsr_render_backward's take decisions (no gradient).  Let z_j = -Z_j
 * be the float gsr_render_aux composites and phi_f,j = d_features[f * n + j].  With
 *   u_j = g_rgb . colour_j + g_A + g_D z_j + sum_f g_f phi_f,j
 * everything gsr_render_backward states holds as written: P_j, G, dL/dalpha_j = T_j u_j -
 * (G - P_j) / (1 - alpha_j), the inactive clamp, d_color, d_opacity, d_conic, d_center.  Two
 * more outputs, both linear:
 *   d_z[i]            += sum over pixels of g_D alpha T     (dL/d(-Z_i))
 *   d_feat[f * n + i] += sum over pixels of g_f alpha T     (dL/d phi_f,i)
 * There is no normalised mode.  A loss on the expected depth D = depth / alpha with gradient g
 * = dL/dD passes d_grad_depth = g / alpha and adds -g depth / alpha^2 to d_grad_alpha.
 *
 * Outputs are planar [c * n + i], ACCUMULATE, and are summed with float atomics: like
 * gsr_render_backward's they are NOT reproducible bit for bit.  An output whose gradient is
 * identically zero for want of an upstream is not touched (d_color without d_grad_image, d_z
 * without d_grad_depth, d_feat without d_grad_feat), nor is a Gaussian no pixel composited.
 * With d_grad_depth, d_grad_feat, d_z and d_feat all NULL and nfeat == 0 the call is
 * gsr_render_backward: the same kernel at the same cost.
 * Frame policy, incomplete frames and GSR_E_OVERFLOW are gsr_render_backward's.  Workspaces
 * are gsr_render_aux's (-Z per Gaussian; the interleaved features above four), grown by
 * high-water mark.  GSR_E_ARG, before any device work: up or out NULL; all four gradient
 * inputs NULL; every output NULL; nfeat outside [0, GSR_AUX_MAX_FEATURES]; nfeat > 0 without
 * d_features; d_grad_feat or out->d_feat with nfeat == 0; the frame arguments gsr_render
 * refuses.
 *
 * gsr_project_backward_aux is gsr_project_backward with an eleventh upstream entry, d_z[i] =
 * dL/d(-Z_i), Z = (V [p, 1])_z: it adds -V[2][j] d_z to the position gradient, and through the
 * position to trbf_center and the motion arrays of a 4D block.  A Gaussian is skipped when all
 * ELEVEN entries are +-0; every other rule, the reproducibility and the argument errors are
 * gsr_project_backward's ("every input NULL" counts five).  With d_z NULL it is
 * gsr_project_backward bit for bit.
 *
 * gsr_render_backward_scene_aux is the fused call over ELEVEN record planes (colour 3,
 * opacity 1, conic 4, centre 2, z 1: the first ten where gsr_render_backward_scene has them),
 * in d_record_scratch or a workspace of the context (11 n floats through this call only),
 * zeroed on `stream` first.  Feature gradients have no scene array to go to: they are added to
 * d_feat_grad (nfeat planes of n floats, ACCUMULATED, or NULL).  Errors as the two calls'. */
typedef struct gsr_aux_upstream {      /* inputs */
    const float* d_grad_image;  /* 3*W*H or NULL */
    const float* d_grad_alpha;  /* W*H or NULL */
    const float* d_grad_depth;  /* W*H or NULL */
    const float* d_grad_feat;   /* nfeat*W*H planar or NULL */
    const float* d_features;    /* nfeat arrays of n floats, as gsr_aux_targets; NULL iff nfeat == 0 */
    int          nfeat;         /* 0..GSR_AUX_MAX_FEATURES */
} gsr_aux_upstream;
typedef struct gsr_record_grads_aux_out {  /* outputs, planar [c*n+i], ACCUMULATED, NULL = not computed */
    float* d_color;    /* 3 planes */
    float* d_opacity;  /* 1 */
    float* d_conic;    /* 4 */
    float* d_center;   /* 2 */
    float* d_z;        /* n floats: dL/d(-Z) */
    float* d_feat;     /* nfeat planes of n floats */
} gsr_record_grads_aux_out;
typedef struct gsr_record_grads_aux {      /* inputs of the projection; NULL = zeros */
    const float* d_color;    /* 3 planes */
    const float* d_opacity;  /* 1 */
    const float* d_conic;    /* 4 */
    const float* d_center;   /* 2 */
    const float* d_z;        /* 1 */
} gsr_record_grads_aux;
int gsr_render_backward_aux(gsr_context* ctx, const void* d_scene, int layout, int64_t n, const gsr_camera* cam,
                            int W, int H, int num_tile_x, int num_tile_y, int width_stride, int height_stride,
                            float k, const gsr_aux_upstream* up, const gsr_record_grads_aux_out* out, void* stream);
int gsr_project_backward_aux(gsr_context* ctx, const void* d_scene, int layout, int64_t n, const gsr_camera* cam,
                             int W, int H, float k, const gsr_record_grads_aux* in, const gsr_scene_grads* out,
                             void* stream);
int gsr_render_backward_scene_aux(gsr_context* ctx, const void* d_scene, int layout, int64_t n,
                                  const gsr_camera* cam, int W, int H, int num_tile_x, int num_tile_y,
                                  int width_stride, int height_stride, float k, const gsr_aux_upstream* up,
                                  float* d_feat_grad /* nfeat planes of n floats, ACCUMULATED, or NULL */,
                                  float* d_record_scratch /* 11 planes of n floats, or NULL */,
                                  const gsr_scene_grads* out, void* stream);

/* Offline camera path (config 4 on one GPU; the reference has no batch entry
 * point — it renders one frame per preprocessCUDAGaussians call, render.cu:871):
 * frame i renders cams[i] (at times[i] for 4D scenes; times may be NULL) into
 * the DEVICE buffer d_outs[i], each frame exactly as gsr_render would.  Up to
 * gsr_set_frames_in_flight() frames run concurrently: frame i goes to lane
 * i % F, lane 0 being this context on `stream` and lanes 1..F-1 private child
 * contexts (own workspaces) on their own streams, so one frame's latency-bound
 * sort and binning kernels overlap another frame's VALU-bound blend.
 * Stream-ordered: the frames start after the work already queued on `stream`
 * (fork event), and work queued on `stream` after the call sees all nframes
 * images (join events).  Outputs may repeat (e.g. a ring of buffers); a frame
 * whose output an in-flight frame of another lane also writes waits for it.
 * Readbacks, timing and diagnostics refer to lane 0's last frame.  Returns
 * GSR_E_OVERFLOW when an earlier frame of any lane was incomplete (see
 * GSR_E_OVERFLOW; every frame since the last clean return re-renders). */
#define GSR_MAX_FRAMES_IN_FLIGHT 8
int gsr_render_path(gsr_context* ctx, const void* d_scene, int layout, int64_t n, const gsr_camera* cams,
                    const float* times, int nframes, int W, int H, int num_tile_x, int num_tile_y,
                    int width_stride, int height_stride, float k, float* const* d_outs, void* stream);
/* gsr_render_path with per-frame completion events, for consumers that hand each
 * finished frame on (the multi-GPU gather) while later frames still render.
 * frame_events (may be NULL; entries may be NULL): hipEvent_t frame_events[i] is
 * recorded on frame i's lane right after its blend.  flags & GSR_PATH_NO_JOIN:
 * skip the join, so `stream` orders after lane 0's frames only and the lanes keep
 * running into the next call without a pipeline drain (a later call's lanes still
 * start after the work queued on `stream` before it).  Without the join the caller
 * orders everything else through the events: reading frame i, and re-using one of
 * this call's output buffers in a later call (wait for the buffer's last frame). */
#define GSR_PATH_NO_JOIN 1
/* flags & GSR_PATH_NO_FORK: lanes 1..F-1 do not wait for `stream` (lane 0 still runs
 * on it), so they are never held behind lane 0's frames of an earlier call (with the
 * fork, chunked calls cost ~4 % of the in-flight rate); the caller orders the frames
 * after its own work through wait_events instead. */
#define GSR_PATH_NO_FORK 2
/* wait_events (may be NULL; entries may be NULL): frame i's lane waits for
 * hipEvent_t wait_events[i] before rendering frame i (e.g. the hand-off of the frame
 * that last used d_outs[i]). */
int gsr_render_path_ex(gsr_context* ctx, const void* d_scene, int layout, int64_t n, const gsr_camera* cams,
                       const float* times, int nframes, int W, int H, int num_tile_x, int num_tile_y,
                       int width_stride, int height_stride, float k, float* const* d_outs, void* stream,
                       void* const* frame_events, void* const* wait_events, int flags);
/* gsr_render_path_ex with a validity word per frame, so a consumer that receives
 * frames asynchronously (the multi-GPU gather) knows exactly which ones to render
 * again instead of every frame since the last clean return.  d_status (may be NULL;
 * entries may be NULL): a uint32 DEVICE word per frame, written on frame i's lane
 * before its frame event: 0 if frame i is complete, else GSR_FRAME_* bits (the causes
 * of GSR_E_OVERFLOW, for that frame alone).  The word can sit right after the
 * frame's image in one buffer, so it travels with the frame.  The return code, the
 * buffer growth and the controller are exactly those of gsr_render_path_ex. */
#define GSR_FRAME_PAIR_OVERFLOW 1u   /* its pairs overflowed the pair buffer */
#define GSR_FRAME_DEPTH_PASSES 2u    /* its depth sort needed more passes than were launched */
#define GSR_FRAME_SPEC_MISS 4u       /* speculative depth-split frame that needed phase B */
int gsr_render_path_status(gsr_context* ctx, const void* d_scene, int layout, int64_t n, const gsr_camera* cams,
                           const float* times, int nframes, int W, int H, int num_tile_x, int num_tile_y,
                           int width_stride, int height_stride, float k, float* const* d_outs, void* stream,
                           void* const* frame_events, void* const* wait_events, int flags,
                           uint32_t* const* d_status);
/* Frames in flight for gsr_render_path: 1..GSR_MAX_FRAMES_IN_FLIGHT (default 3;
 * 1 = strictly sequential on `stream`).  Each extra lane holds its own workspace. */
int gsr_set_frames_in_flight(gsr_context* ctx, int frames);
int gsr_frames_in_flight(gsr_context* ctx);

/* The three stages of gsr_render, callable separately (same stream). */
int gsr_preprocess(gsr_context* ctx, const void* d_scene, int layout, int64_t n,
                   const gsr_camera* cam, int W, int H, int num_tile_x, int num_tile_y,
                   int width_stride, int height_stride, float k, void* stream);
int gsr_sort(gsr_context* ctx, void* stream);
int gsr_blend(gsr_context* ctx, float* d_out, void* stream);

/* Frame time t for GSR_LAYOUT_SCENE_BLOCK_4D scenes (config 5):
 * dt = t - trbf_center; position = xyz + m0..2*dt + m3..5*dt^2 + m6..8*dt^3;
 * opacity = sigmoid(opacity) * exp(-(dt / trbf_scale)^2).  Gaussians whose
 * temporal opacity is below 0.9e-3 (and whose 2D conic is robustly positive
 * definite) are culled in preprocess: they could never reach alpha >= 1e-3,
 * so the image equals the uncut render. */
int gsr_set_time(gsr_context* ctx, float t);

/* Wait for all work of the context (every lane); returns GSR_E_OVERFLOW if any
 * frame since the last clean check was incomplete — including one that a
 * non-blocking check inside a render call already reported — and grows the
 * buffer / resets the pass budget. */
int gsr_sync(gsr_context* ctx);

/* ---- readback (synchronous; for tests and tooling) ---- */

/* Number of (tile, Gaussian) pairs of the last frame's tile rects (before the capacity
 * clamp; an upper bound of the pairs listed when GSR_TUNE_TILE_SPANS drops some). */
int64_t gsr_pair_count(gsr_context* ctx);
/* Number of (tile row, Gaussian) items the last frame's row pass produced (tile
 * binning), or -1 if that frame used pair emission + the key-value tile sort. */
int64_t gsr_row_item_count(gsr_context* ctx);
/* Per-Gaussian splat records (n * GSR_SPLAT_RECORD_BYTES bytes):
 *   float inv_covar[4]; float opacity; float color[3];
 *   int32 px_x, px_y; uint32 x_range (xmin | xmax<<16); uint32 y_range;
 *   uint32 tile_x_range; uint32 tile_y_range; uint32 tile_count; uint32 depth_key.
 * Culled / invalid Gaussians have tile_count 0 and depth_key 0xFFFFFFFF;
 * their other fields are unspecified. */
int gsr_read_splats(gsr_context* ctx, void* host_records, int64_t n);
/* (depth_key << 32 | index) items after the depth sort, n of them.  A frame
 * that used the per-tile depth order has no global one: it is computed here
 * (stable sort of that frame's keys, the same kernels as the global path). */
int gsr_read_depth_order(gsr_context* ctx, uint64_t* host_items, int64_t n);
/* (tile << 32 | index) pairs the tile lists hold, in tile order; returns the count copied. */
int64_t gsr_read_pairs(gsr_context* ctx, uint64_t* host_pairs, int64_t cap);
/* Internal tile grid of the last frame and its [start, end) ranges. */
int gsr_tile_grid(gsr_context* ctx, int* tiles_x, int* tiles_y);
int gsr_read_tile_ranges(gsr_context* ctx, uint32_t* host_ranges, int64_t num_tiles);

/* ---- per-stage device timing with hipEvents on the render stream ----
 * mode 0 = off, 1 = blend only (two events per frame), 2 = every stage. */
int gsr_set_timing(gsr_context* ctx, int mode);
/* Same, recording the events on every `stride`-th frame only (frames 0, k, 2k, …
 * after the call); gsr_stage_times then averages over the recorded frames. */
int gsr_set_timing_stride(gsr_context* ctx, int mode, int stride);
/* Sums of per-stage device milliseconds and the number of frames timed since
 * the last call (synchronises, then resets). */
int gsr_stage_times(gsr_context* ctx, double* ms_out /* GSR_NUM_STAGES */, int64_t* frames);

/* Diagnostics (off by default): when on, the blend counts the splat records
 * it actually loads (Pc of SURVEY.md 8d: pairs consumed before every pixel of
 * a tile saturates); gsr_blend_records_loaded() returns the last frame's Pc. */
int gsr_set_diagnostics(gsr_context* ctx, int on);
int64_t gsr_blend_records_loaded(gsr_context* ctx);
/* All blend counters of the last diagnostics frame (8 values): {records
 * loaded (Pc), wave-splat iterations, active lanes (in AABB and not
 * saturated), lanes that composited, iterations on the exact one-splat
 * path (default schedule; batches without the fast-path proof),
 * iterations skipped by the per-splat md2 cutoff (variant 5), pixel-lane slots
 * (64 x pixels per lane x iterations), 0};
 * lane efficiency = active / slots. */
int gsr_blend_counters(gsr_context* ctx, int64_t* out8);
/* The first n (<= 16) blend counters: the 8 above, then {blocks the fast-exp blend
 * handed to the exact blend, their suspect pixels}. */
int gsr_blend_counters_ex(gsr_context* ctx, int64_t* out, int n);
/* Take map of the last diagnostics frame: per pixel (row-major, n = W * H), the
 * number of splats composited (low 32 bits) and the sum over them of
 * (gaussian index + 1) * 2654435761 mod 2^32 (high 32 bits).  The oracle's
 * orc_render_takes computes the same map, so the tests compare which splats
 * every pixel composited, not only the colours. */
int gsr_blend_take_map(gsr_context* ctx, uint64_t* out, int64_t n);
/* Blend schedule: 0 = one 64-thread workgroup per 8x8 pixel block (the
 * kernel); 3 = the same with per-wave timestamps instead of counters (see
 * gsr_blend_stamps; diagnostics frames only).  Other values are refused (the
 * tile-per-workgroup schedule, longest-tiles-first, several blocks per wave or
 * workgroup and LDS-capped occupancy were measured slower and removed). */
int gsr_set_blend_variant(gsr_context* ctx, int variant);
/* Tuning knobs for A/B experiments (all settings give bit-identical output, except
 * GSR_TUNE_BLEND_EXP: its modes composite the same splats on every pixel and differ in
 * the colours by < 1e-6). */
enum {
    GSR_TUNE_BLEND_SCHEDULE = 0,     /* as gsr_set_blend_variant */
    GSR_TUNE_TILE_SORT_ITEMS = 1,    /* tile sort items per thread: 8 | 16 (default 16) */
    GSR_TUNE_DEPTH_SORT_ITEMS = 2,   /* depth sort items per thread: 0 = by size | 8 | 16 (16 sorts one
                                        4,096-item tile per workgroup: a grid too small for that, e.g.
                                        capped by knob 4, sorts 8 per thread) */
    GSR_TUNE_TILE_SORT_GROUPS = 3,   /* tile sort workgroup cap (default 1024; 0 = one per tile of items) */
    GSR_TUNE_DEPTH_SORT_GROUPS = 4,  /* depth sort workgroup cap (0 = one per tile of items) */
    GSR_TUNE_TILE_SORT_SPLIT = 5,    /* tile sort digits: 1 = split evenly (default), 0 = 8 bits first */
    GSR_TUNE_DEPTH_SORT_SKIP = 6,    /* depth sort: 1 = skip trailing identity passes (default), 0 = run all 4 */
    GSR_TUNE_TILE_BINNING = 7,       /* 1 = row + column binning (default; tile grids <= 256 x 256),
                                        0 = pair emission + key-value tile sort */
    GSR_TUNE_BIN_ROW_ITEMS = 8,      /* binning row pass: items per thread per tile 4 | 8 | 16 (default 4) */
    GSR_TUNE_BIN_COL_ITEMS = 9,      /* binning column pass: items per thread per tile 4 | 8 | 16 (default 8) */
    GSR_TUNE_BIN_COL_GROUPS = 10,    /* binning column pass: workgroups (default 0 = n / 1024 clamped
                                        to 1024..4096) */
    GSR_TUNE_COMPLETION_EVENTS = 11, /* 1 (default): a completion event feeds the non-blocking overflow
                                        check; 0: none (frames captured into a graph).  With 0 the
                                        render calls report nothing: only gsr_sync (which drains the
                                        device, then reads the sticky overflow words) reports an
                                        incomplete frame, and no frame is rendered speculatively
                                        without the depth split's phase B (a graph would replay that
                                        choice) */
    /* 12 reserved (removed: longest tiles first) */
    GSR_TUNE_BLEND_BAND_TILES = 13,  /* blend schedule 0: tiles per spatial band, bands dealt round-robin
                                        to the 8 XCDs (default 4); 0 = one contiguous band per XCD */
    /* 14-17 reserved (removed, all measured slower: two blocks per workgroup, per-tile depth
       order after index-order binning (config 3: 1.53 ms vs 0.24 ms), several blocks per wave,
       LDS-capped blend occupancy) */
    GSR_TUNE_DEPTH_COMPACT = 18,     /* global depth sort on the binning path: 1 = stable partition of the
                                        visible Gaussians first, the passes sort only those; 0 = sort all;
                                        2 (default) = partition for 4D scenes only; same order, same image */
    GSR_TUNE_TILE_SPANS = 19,        /* binning path: 1 = list a splat in only the tiles of its first four
                                        tile rows it can composite on (conservative ellipse-vs-tile test);
                                        0 = every tile of its rect; 2 (default) = 1 up to 1.5M Gaussians;
                                        same image */
    GSR_TUNE_RANK_ATOMIC = 20,       /* stable digit ranks in the depth sort and both binning scatters:
                                        1 (default) = from returning LDS atomics, taken only on a gfx950
                                        device that passed the one-shot rank-order self-check
                                        (gsr_rank_order_check) when the context first ran; 0 = ballot
                                        matching.  The environment variable GSR_RANK_ATOMIC=0 makes 0
                                        the default.  Same order, same image */
    GSR_TUNE_RANK_ATOMIC_ACTIVE = 21, /* read-only: 1 if the atomic ranks are in use (knob 20 at 1 and the
                                        self-check passed), 0 if the kernels rank with ballots */
    GSR_TUNE_BLEND_EXP = 22,         /* blend exp.  1 (default since round 4) = hardware exp for
                                        alpha, with the alpha test exact on the exp argument and the
                                        transmittance test guarded by a proven band; pixels whose T
                                        decision the band cannot vouch for are blended again exactly.
                                        Every pixel composites exactly the oracle's splats (take map
                                        identical); colours within 1e-6 of the exact blend (measured
                                        <= 4e-7).  0 (environment GSR_BLEND_EXP=0 selects it) =
                                        gsr_blend_expf throughout: bit-exact with the oracle.  Depth-
                                        split frames (GSR_TUNE_DEPTH_SPLIT) always run the exact blend.
                                        2 = test hook: 1 with a 100 % guard band, so every block
                                        in which a pixel saturates is blended again exactly. */
    GSR_TUNE_DEPTH_SPLIT = 23,       /* binning path, exact blend, gsr_render / gsr_render_path: 1 = bin
                                        the nearest part of the depth order first and blend it (phase
                                        A), then bin the rest and resume only the 8x8 blocks phase A
                                        left unsaturated (phase B, skipped on the device when there are
                                        none).  After the first split frame the items are partitioned
                                        by a depth threshold and only the near part is sorted (phase B
                                        sorts the far part when it runs); the split point adapts to the
                                        frames seen, and once it cannot shrink further frames are
                                        rendered without phase B until one needs it (that frame returns
                                        GSR_E_OVERFLOW: render it again).  A split point grown to 1000
                                        turns it off; it is tried again 256+ frames later, only on
                                        another camera.  0 = one phase; 2 (default) =
                                        1 above 1.5M Gaussians.  Same image.  After a split frame
                                        gsr_read_pairs / gsr_read_tile_ranges hold the lists of its last
                                        phase, and after a threshold split gsr_read_depth_order is refused */
    GSR_TUNE_DEPTH_SPLIT_PERMILLE = 24, /* the current split point: phase A bins the nearest
                                        ceil(n * value / 1000) of the depth order (adapted per frame; a
                                        set value is a new starting point, 1..999) */
    GSR_TUNE_DEPTH_SPLIT_UNSAT = 25, /* read-only: 8x8 blocks the last completed split frame's phase A
                                        left unsaturated (0: its phase B did nothing); read after gsr_sync */
    GSR_TUNE_DEPTH_SPLIT_STATE = 26, /* read-only: how the last sorted frame ran: 0 one phase; 1 split,
                                        whole depth order sorted (count mode: the first split frame);
                                        2 split by a depth threshold (near part sorted, far part sorted
                                        in phase B); 3 as 2 with no phase B queued (speculative: a frame
                                        that then leaves a block unsaturated is reported as
                                        GSR_E_OVERFLOW and rendered again by the caller).  Aux frames
                                        (gsr_render_aux, always one phase) do not count: the knob keeps
                                        the value of the frame before them */
    /* 27 reserved (removed, measured slower: the preprocess building the depth sort's pass-0
       histograms in 512-thread workgroups of 2048 Gaussians, pass 0 without its upsweep launch:
       preprocess 49.4 -> 60.3 us against the 5.7-us upsweep, -1.1 % one frame at a time and
       -1.2 % in flight, profiles/r04_ab_pre_hist.txt) */
    GSR_TUNE_DEPTH_BUCKETS = 28,     /* binning path, frames not split by a depth threshold: 1 (default) =
                                        bucket depth sort: one stable scatter of the preprocess order into
                                        depth buckets bounded by the previous frame's quantiles, then one
                                        workgroup per bucket sorts it in LDS.  Up to 2,097,152 Gaussians
                                        ~n/1024 buckets (at most 4,096) of up to 2,048 items per 256-thread
                                        workgroup (larger buckets are sorted through global memory by their
                                        workgroup); above, 512 buckets of up to 16,384 items per 1,024-thread
                                        workgroup (larger or wider-keyed ones go to the first kind's
                                        paths in a second launch).  A context's first frame of a scene size
                                        runs the LSD passes and takes the quantiles from them, and so does
                                        the first frame of another scene pointer, and the frame after one
                                        whose global path ran more than n/8 item-passes (a camera cut; knob
                                        33).  0 = LSD passes only; 2 = test hook: 1 with a 64-item local
                                        capacity in either kind (no reseeding on overflow); 3 = the first
                                        kind at any scene size (A/B).  Same order, same image;
                                        gsr_depth_passes is 0 after a bucket-sorted frame */
    GSR_TUNE_DEPTH_BUCKETS_OVER = 29, /* read-only: items the bucket sort's global path has sorted (buckets
                                        over the local capacity), summed over the lanes; sticky, read
                                        after gsr_sync */
    GSR_TUNE_BUCKET_ROWS = 30,       /* 1 (default): on a bucket-sorted frame binned once over the whole
                                        depth order, each bucket's workgroup also counts the row pass's
                                        items and pairs (the bucket is the row pass's chunk), so the row
                                        pass runs without its count kernel; 0 = the row pass counts.
                                        Same lists, same image */
    GSR_TUNE_COL_CHUNK = 31,         /* binning path: row items per column-pass chunk.  0 (default) =
                                        1024 for scenes of at most 2,097,152 Gaussians, else 2048;
                                        1024 or 2048 forces it.  Same lists, same image */
    GSR_TUNE_FAIL_FRAME = 32,        /* test hook: v > 0 makes the next gsr_render_path* call fail its
                                        frame v with GSR_E_ARG (once; 0 = off, the default).  The
                                        frames queued before it are still joined to the caller's
                                        stream */
    GSR_TUNE_DEPTH_BUCKETS_WORK = 33,/* read-only: the global path's items times the 8-bit passes each
                                        took (their bucket's key span; tied keys take none), summed
                                        over the lanes; sticky, read after gsr_sync.  A frame adding
                                        more than n/8 makes the next frame reseed the splitters */
    GSR_TUNE_PATH_SHARED_PRE = 34,   /* gsr_render_path*: 1 (default) = the frames in flight of a group
                                        (one per lane) share one preprocess launch that reads the scene
                                        once for up to four cameras (3D scene blocks, with or without
                                        SH-3, depth split off, no diagnostics, no per-stage timing;
                                        anything else keeps one launch per frame); each lane then holds
                                        a second set of preprocess outputs, ~82 B per Gaussian, from
                                        the first shared group on.  The shared launch runs on the
                                        caller's stream and waits for the wait_events of the group's
                                        frames.  0 = one launch per frame.  Same records, same image */
    GSR_TUNE_PATH_SHARED_LAUNCHES = 35 /* read-only: shared preprocess launches this context has issued */
};
int gsr_set_tuning(gsr_context* ctx, int knob, int value);
/* Current value of a knob (what gsr_set_tuning last set, else the default). */
int gsr_get_tuning(gsr_context* ctx, int knob, int* value);
/* Device self-check behind GSR_TUNE_RANK_ATOMIC: wave64 instructions whose lanes
 * add to the same LDS address with a returning atomic (ds_add_rtn_u32) on the
 * current device, over 24 digit patterns, compared lane by lane with the stable
 * ranks ballot matching gives.  *lane_ops = lanes checked, *mismatches = lanes
 * whose returned value was out of lane order.  The ISA does not document that
 * order; contexts run this once per process and device and rank with ballots if
 * any lane mismatches or the device is not gfx950.  Synchronous, < 1 ms. */
int gsr_rank_order_check(int64_t* lane_ops, int64_t* mismatches);
/* Depth-sort digit passes the last sorted frame ran (1..4; trailing identity
 * passes are skipped on the device), or a negative error code. */
int gsr_depth_passes(gsr_context* ctx);
/* Bucket depth sort diagnostics (GSR_TUNE_DEPTH_BUCKETS) of the last sorted frame of the
 * context (lane 0 of gsr_render_path): its bucket count B, or 0 when that frame was not
 * bucket-sorted, and each bucket's item count into sizes[0 .. min(B, cap)) (bucket B - 1
 * holds the items with key 0xFFFFFFFF: the culled ones).  Synchronizes the context. */
int gsr_bucket_sizes(gsr_context* ctx, uint32_t* sizes, int cap);
/* Schedule 3: with diagnostics on, the last frame's blend stores per wave
 * (launch order) {start of the 100 MHz s_memrealtime clock, duration (40 bits) |
 * placement << 40 (XCC id, HW_ID)}; read n values. */
int gsr_blend_stamps(gsr_context* ctx, uint64_t* out, int64_t n);

/* ---------------------------------------------------------------- scenes */

/* Upload a host SoA scene (GSR_SCENE_NARRAYS arrays of n floats, contiguous,
 * already activated as by the loader) into a new device scene block. */
void* gsr_scene_upload(const float* host_soa, int64_t n);
/* narrays = GSR_SCENE_NARRAYS (3D), GSR_SCENE4D_NARRAYS (4D) or GSR_SCENE_SH3_NARRAYS. */
void* gsr_scene_upload_ex(const float* host_soa, int narrays, int64_t n);
void gsr_scene_free(void* d_scene);
/* Bytes of a scene block (header + narrays arrays of n floats, padded), or a
 * negative error code. */
int64_t gsr_scene_bytes(int narrays, int64_t n);
/* Copy a whole device scene block (n Gaussians, narrays arrays: checked against its
 * header) into d_dst, a device buffer of gsr_scene_bytes(narrays, n) bytes, on
 * `stream` — e.g. into a buffer that a collective then broadcasts to the other
 * ranks (the multi-GPU scene replication; the copy is a valid scene block). */
int gsr_scene_copy(void* d_dst, const void* d_scene, int narrays, int64_t n, void* stream);
/* Copy a device scene block back into host SoA form (38 * n floats). */
/* Copies every array of the block (38, 49 for 4D, 59 for SH-3) into host_soa. */
int gsr_scene_download(const void* d_scene, float* host_soa, int64_t n);

/* ---- scene editing: new scene blocks from a keep mask or an index list, on the device ----
 *
 * The consumer half of gsr_render_contrib: a selection never edits a scene block in place (the
 * two writers of a block are gsr_scene_adam_step and gsr_scene_reset_opacity, below); these calls build
 * a new one (a pruned scene, a level-of-detail or visibility subset, a reordered scene)
 * without the download / numpy / upload round trip, and cut the caller's per-Gaussian side
 * arrays (gsr_render_aux's feature planes, gsr_render_contrib's accumulators) down in step.
 * All four are context-free.  Indices are int32 (scene sizes are capped at INT32_MAX).
 *
 * A selection (a monotone index list) keeps index order, the depth sort's tie-break, so
 * dropping Gaussians that no pixel composited (d_count == 0) leaves the exact blend's image
 * bit for bit unchanged.
 *
 * Every argument error returns GSR_E_ARG (or NULL with the error set) before any device work:
 * a null pointer, a bad narrays, negative n or m, n or m > INT32_MAX, elem_bytes not 4 or 8,
 * nplanes < 1, a stride smaller than its count, m > 0 with n == 0. */

/* Stable stream compaction: writes the ascending indices i < n with d_keep[i] != 0 (any
 * non-zero byte keeps) into d_indices[0 .. m) and returns m in the HOST word *m_out.
 * d_indices has room for n words; words at m and beyond are left untouched.  Enqueues on
 * `stream`, then waits for it: SYNCHRONOUS, like the readbacks (it allocates and frees n / 1024
 * bytes of scratch).  n == 0 gives m = 0 without device work. */
int gsr_mask_indices(const uint8_t* d_keep, int64_t n, int32_t* d_indices, int64_t* m_out, void* stream);
/* Planar gather: dst[p * dst_stride + j] = src[p * src_stride + d_indices[j]] for p < nplanes,
 * j < m.  Elements are elem_bytes = 4 or 8 bytes, copied as bits; strides are in elements,
 * src_stride >= n and dst_stride >= m; the buffers must not overlap.  Indices may come in any
 * order and may repeat (m > n is legal).  Stream-ordered: no allocation, no wait.
 * The kernel never forms an address from an unchecked index: an index outside [0, n) reads
 * element min(max(index, 0), n - 1) instead, and *d_bad (may be NULL; a device word the caller
 * zeroes) is incremented by the number of such indices.
 * Cost: a monotone list reads every plane in near-coalesced runs and all stores are
 * coalesced; a random permutation pays one cache line per element and plane, which is inherent
 * to the SoA layout ("Scene editing"). */
int gsr_gather_planes(void* d_dst, int64_t dst_stride, const void* d_src, int64_t src_stride, int nplanes,
                      int elem_bytes, int64_t n, const int32_t* d_indices, int64_t m, uint32_t* d_bad,
                      void* stream);
/* A new scene block of m Gaussians (one hipMalloc; free with gsr_scene_free or hipFree):
 * Gaussian j is Gaussian d_indices[j] of d_scene in all narrays arrays; count = m, stride = m
 * rounded up to 64, the same narrays; elements in [m, stride) are unspecified, as after an
 * upload.  d_scene's header is checked against (narrays, n) as gsr_scene_copy does (read
 * synchronously); an AoS array or a mismatching block is refused.  The gather and the new
 * header are written on `stream`: the block is valid for work queued on `stream` after the
 * call.  Out-of-range indices and d_bad as in gsr_gather_planes.  m == 0 gives a header-only
 * block.  Returns NULL and sets gsr_last_error on failure. */
void* gsr_scene_gather(const void* d_scene, int narrays, int64_t n, const int32_t* d_indices, int64_t m,
                       uint32_t* d_bad, void* stream);
/* gsr_mask_indices followed by gsr_scene_gather: the scene of the Gaussians with d_keep[i] != 0,
 * in index order; their number in the HOST word *m_out.  d_indices (may be NULL; room for n
 * words): receives the kept source indices, for compacting side arrays with
 * gsr_gather_planes.  SYNCHRONOUS on `stream` (m must be known before the block is
 * allocated). */
void* gsr_scene_select(const void* d_scene, int narrays, int64_t n, const uint8_t* d_keep, int64_t* m_out,
                       int32_t* d_indices, void* stream);

/* ---- scene optimisation: the call that steps a scene block in place ----
 * (gsr_scene_reset_opacity, under "scene densification", is the only other writer of a block)
 *
 * The update of render -> loss -> gsr_render_backward_scene -> UPDATE -> prune: one fused,
 * in-place Adam step of the block's arrays from gsr_project_backward's gradient planes, so a
 * scene is fine-tuned, or re-fitted after a prune, without leaving the device.  Context-free,
 * stream-ordered: it never allocates, synchronises or reads the block's header, and trusts
 * (layout, n) as gsr_render does.
 *
 * grads are gsr_project_backward's outputs; m and v, the first and second moments, have the
 * same shapes (planar [c*n + i], the block's array order), are owned by the caller, zeroed
 * once, and cut down with the scene by gsr_gather_planes after a prune.
 *
 * Groups, each with its own learning rate: d_position (lr_position), d_opacity (lr_opacity),
 * d_scale (lr_scale), d_rot (lr_rot); d_sh is two groups, its first 3 planes the dc
 * coefficients (lr_sh_dc) and its other 24 (45 for an SH-3 block) the rest (lr_sh_rest);
 * d_temporal is three, plane 0 trbf_center (lr_tcenter), plane 1 trbf_scale (lr_tscale),
 * planes 2..10 the motion arrays (lr_motion).  A group is ACTIVE when its gradient pointer is
 * non-NULL and its lr is not 0; a frozen group is neither read nor written, and its moment
 * pointers may be NULL.
 *
 * The block stores the opacity as sigmoid(raw) and the scales and trbf_scale as exp(raw); the
 * gradients are with respect to the stored values.  The step is the 3DGS parametrisation's, in
 * raw space, written without a log.  Per element, in float32, every operation rounded once
 * (no FMA), in exactly this order — with omb1 = 1 - beta1, omb2 = 1 - beta2, bc1 = 1 -
 * pow(beta1, step), bc2 = 1 - pow(beta2, step) computed by the host in double from the float
 * betas and rounded to float:
 *   g' = g * chain       chain = 1 for the plain arrays (g' = g),
 *                        o * (1 - o) for the opacity, s for the scales and trbf_scale
 *   m' = (beta1 * m) + (omb1 * g')
 *   v' = (beta2 * v) + ((omb2 * g') * g')
 *   d  = (lr * (m' / bc1)) / (sqrtf(v' / bc2) + eps)
 *   position, rot, sh, trbf_center, motion:   x' = x - d
 *   scale, trbf_scale:                        s' = s * gsr_expf(-d)           (log s - d)
 *   opacity:   o' = o / (o + (1 - o) * gsr_expf(d))                           (logit o - d)
 *              then fminf(fmaxf(o', GSR_ADAM_OPACITY_MIN), GSR_ADAM_OPACITY_MAX)
 * gsr_expf is gsr_detmath.h's.  The quaternion is stepped raw (its gradient already runs
 * through the normalisation).
 *
 * Skipped elements keep their bits in x, m and v:
 *   - g not finite: skipped, and *d_bad (may be NULL; a device word the caller zeroes) is
 *     incremented by the number of such elements;
 *   - with GSR_ADAM_SKIP_ZERO, g = +-0: skipped.  gsr_project_backward never touches a
 *     Gaussian that no pixel composited, so this is the visible-only ("sparse") Adam: the
 *     moments of what a batch did not see do not decay.  A wave whose gradients are all zero
 *     loads nothing else.
 * With GSR_ADAM_ZERO_GRADS every element of every active group's gradient planes reads +-0
 * after the call, the skipped ones included: the batch's memset pass is saved.
 *
 * One thread owns one element, no atomics but *d_bad: reproducible bit for bit.  Elements
 * [n, stride) of the block, and everything past n in any plane, are never read or written.
 * The step is ordered on `stream`: frames of gsr_render_path* still in flight on other lanes
 * must have joined it first (the default join does; with GSR_PATH_NO_JOIN wait on the frame
 * events).  A stepped block renders through an existing context like any other frame: no
 * context state holds scene contents.
 * GSR_E_ARG, before any device work: d_scene NULL with n > 0; grads, m, v or cfg NULL;
 * GSR_LAYOUT_AOS or an unknown layout; n outside [0, INT32_MAX]; no active group; an active
 * group without both moment planes; d_temporal active on a block that is not 4D; an lr that is
 * negative or not finite; beta1 or beta2 outside [0, 1); eps not finite or <= 0; step < 1;
 * unknown flag bits; a pointer that is not 4-byte aligned.  n == 0 is GSR_OK without device
 * work. */
enum { GSR_ADAM_SKIP_ZERO = 1, GSR_ADAM_ZERO_GRADS = 2 };
#define GSR_ADAM_OPACITY_MIN 1e-6f
#define GSR_ADAM_OPACITY_MAX 0.999999f
typedef struct gsr_adam_config {
    float lr_position, lr_opacity, lr_scale, lr_rot, lr_sh_dc, lr_sh_rest;   /* 3D groups */
    float lr_tcenter, lr_tscale, lr_motion;                                  /* 4D blocks only */
    float beta1, beta2, eps;
    int64_t step;      /* t >= 1, for the bias correction */
    int flags;         /* GSR_ADAM_* */
} gsr_adam_config;
int gsr_scene_adam_step(void* d_scene, int layout, int64_t n,
                        const gsr_scene_grads* grads,   /* gsr_project_backward's outputs */
                        const gsr_scene_grads* m, const gsr_scene_grads* v,   /* moments, same shapes, caller-owned */
                        const gsr_adam_config* cfg, uint32_t* d_bad, void* stream);

/* ---- scene densification: clone, split and prune on the device ----
 *
 * The GROW step of render -> loss -> gsr_render_backward_scene -> gsr_scene_adam_step ->
 * densify / prune: 3DGS's adaptive density control.  Small Gaussians with a large screen-space
 * position gradient are cloned, large ones are split in two, and transparent or oversized
 * ones are dropped, without the download / numpy / upload round trip.  All calls are
 * context-free.
 *
 * 1. The statistic.  gsr_densify_accumulate reads the two centre planes gsr_render_backward
 * wrote (d_center; planes 8 and 9 of gsr_render_backward_scene's record scratch): gx =
 * d_center[i], gy = d_center[n + i].  Per Gaussian:
 *   - gx and gy both +-0: not touched (no pixel composited it: gsr_project_backward's rule);
 *   - gx or gy not finite: not touched, and *d_bad (may be NULL; a device word the caller
 *     zeroes) is incremented;
 *   - otherwise, in float32 with one rounding per operation,
 *       a = gx * (0.5f * W),  b = gy * (0.5f * H)
 *       d_grad_accum[i] += sqrtf((a * a) + (b * b)),  d_seen[i] += 1
 *     W/2 and H/2 turn the pixel gradient into the NDC units of 3DGS's threshold 0.0002.
 * Both arrays (n words each) ACCUMULATE and are never cleared by the library: the caller
 * zeroes them once and again after every densify.  One thread owns one Gaussian, no atomics
 * but *d_bad: reproducible bit for bit.  Stream-ordered, never allocates.
 * GSR_E_ARG, before any device work: a NULL d_center, d_grad_accum or d_seen with n > 0; n
 * outside [0, INT32_MAX]; W or H < 1; a pointer that is not 4-byte aligned.  n == 0 is GSR_OK
 * without device work. */
int gsr_densify_accumulate(const float* d_center /* 2 planes of n floats */, int64_t n, int W, int H,
                           float* d_grad_accum /* n, ACCUMULATED */, uint32_t* d_seen /* n, ACCUMULATED */,
                           uint32_t* d_bad /* or NULL */, void* stream);

/* 2. The densify call.  For source i, every comparison in float32 as written (NaNs compare
 * false):
 *   avg   = d_seen[i] ? d_grad_accum[i] / (float)d_seen[i] : 0
 *   hot   = avg >= grad_threshold
 *   smax  = fmaxf(fmaxf(scale0, scale1), scale2) of the stored scales
 *   split = hot && smax > scale_split,   clone = hot && !split
 * A kept source emits itself (kind 0); a cloned one itself (kind 0) and then a bit-identical
 * copy (kind 1); a split one its two children (kinds 2 and 3) and not itself.  The prune
 * tests are applied to an output's own values, as 3DGS prunes after it has densified:
 *   sout   = split ? smax / split_shrink : smax
 *   pruned = stored opacity < min_opacity || sout > prune_scale_max
 * (a child keeps its parent's opacity), so all outputs of a source share one fate and a source
 * emits 0, 1 or 2 Gaussians.  Outputs appear in source index order, one source's outputs
 * adjacent: one exclusive scan places them, and children stay beside their parent's neighbours
 * in the preprocess order (the depth sort's tie-break).
 *
 * A split child (k = 0 for kind 2, k = 1 for kind 3) copies every array of its parent — SH,
 * rotation, opacity, the temporal arrays of a 4D block — except the scales and the position:
 *   s'_c = s_c / split_shrink
 *   t_c  = z_c * s_c                     (s the PARENT's scales)
 *   p'_r = p_r + ((R[r][0] * t0 + R[r][1] * t1) + R[r][2] * t2)
 * R the rotation matrix of the normalised quaternion, by the preprocess's own expressions
 * (math.cu:153-164), and (z0, z1, z2) = gsr_densify_normals(seed, i, k): the child's sample
 * depends on (seed, i, k) alone, not on the other Gaussians' fates, the output position or the
 * launch shape.  Non-finite values propagate without a special case.
 *
 * The result is a new scene block as gsr_scene_gather builds it (one hipMalloc; count n_out,
 * stride rounded up to 64, the same narrays; free with gsr_scene_free); n_out == 0 gives a
 * header-only block.  d_src[j] (may be NULL; room for 2n words) receives output j's source and
 * d_kind[j] (may be NULL; room for 2n bytes) its kind; entries at n_out and beyond are left
 * untouched.  *report (host) counts the SOURCES by fate — kept + cloned + split + pruned = n,
 * n_out = kept + 2 (cloned + split) — and is written only on success.
 * SYNCHRONOUS on `stream`, like gsr_scene_select (n_out must be known before the block is
 * allocated); allocates and frees its own scratch (n / 256 bytes, and the lists the caller
 * did not pass).  Everything is integer or one-owner arithmetic: reproducible bit for
 * bit.  d_scene's header is checked against (narrays, n) as gsr_scene_select does.
 * Returns NULL and sets gsr_last_error on failure.  GSR_E_ARG, before any device work: the
 * cases gsr_scene_select refuses (a NULL d_scene, a bad narrays, n outside [0, INT32_MAX]); n >
 * INT32_MAX / 2; a NULL cfg or report, or with n > 0 a NULL d_grad_accum or d_seen; a NaN
 * field in cfg; grad_threshold or scale_split negative; min_opacity outside [0, 1];
 * prune_scale_max <= 0; split_shrink not finite or <= 1; unknown flag bits. */
typedef struct gsr_densify_config {
    float grad_threshold;   /* hot when accum / seen >= this (3DGS 0.0002); +inf: nothing is hot */
    float scale_split;      /* hot and max scale >  this: split;  hot and <= this: clone (3DGS: 0.01 * scene extent) */
    float min_opacity;      /* outputs with stored opacity < this are dropped (3DGS 0.005); 0: off */
    float prune_scale_max;  /* outputs with max scale > this are dropped (3DGS: 0.1 * extent); +inf: off */
    float split_shrink;     /* a split child's scales are the parent's / this (3DGS 1.6 = 0.8 * 2) */
    uint64_t seed;
    int flags;              /* 0; unknown bits refused */
} gsr_densify_config;
typedef struct gsr_densify_report { int64_t n_out, kept, cloned, split, pruned; } gsr_densify_report; /* sources by fate */
void* gsr_scene_densify(const void* d_scene, int narrays, int64_t n, const float* d_grad_accum, const uint32_t* d_seen,
                        const gsr_densify_config* cfg, int32_t* d_src /* room for 2n, or NULL */,
                        uint8_t* d_kind /* room for 2n, or NULL */, gsr_densify_report* report /* host */, void* stream);

/* 3. The sampler, on the host: out3 = the three normals of child `child` of source `index`
 * under `seed` — the host build of the code the split kernel runs (gsr_densify_normal3,
 * gsr_detmath.h: Philox4x32-10 at counter (index, child, 0, 0) under key (seed low word, seed
 * high word), then Box-Muller on gsr_logf, gsr_cosf and gsr_sinf), bit for bit what the device
 * draws.  gsr_logf_probe: out[i] = gsr_logf(in[i]) for n host floats (positive normal values),
 * for the accuracy sweep of the tests; GSR_E_ARG for a NULL pointer or n < 0. */
void gsr_densify_normals(uint64_t seed, uint32_t index, uint32_t child, float out3[3]);
int gsr_logf_probe(const float* host_in, int n, float* host_out);

/* 4. Companions.
 * gsr_densify_gather_planes cuts the Adam moments over to a densified scene in one call:
 *   dst[p * dst_stride + j] = d_kind[j] ? +0 : src[p * src_stride + d_src[j]],  p < nplanes, j < m
 * over float planes — survivors (kind 0) keep their moments and every new Gaussian starts at
 * zero, as 3DGS does.  An index is read only where d_kind[j] == 0; there gsr_gather_planes'
 * rule holds: no address is formed from an unchecked index, an index outside [0, n) reads
 * element min(max(index, 0), n - 1) and *d_bad (may be NULL) counts it.  Stream-ordered, no
 * allocation.  GSR_E_ARG as gsr_gather_planes (with elem_bytes 4), and for a NULL d_kind. */
int gsr_densify_gather_planes(float* d_dst, int64_t dst_stride, const float* d_src_planes, int64_t src_stride,
                              int nplanes, int64_t n, const int32_t* d_src, const uint8_t* d_kind, int64_t m,
                              uint32_t* d_bad, void* stream);
/* gsr_scene_reset_opacity: 3DGS's periodic opacity reset, the second call that writes to a
 * scene block.  In place, o' = fminf(o, cap) for i < n (a NaN opacity becomes cap), and
 * d_m_opacity[i] = d_v_opacity[i] = +0 for i < n (the opacity group's Adam moments; each may be
 * NULL).  Elements [n, stride) and every other array keep their bits.  Stream-ordered, never
 * allocates, synchronises or reads the block's header: it trusts (layout, n) as
 * gsr_scene_adam_step does, and is ordered on `stream` under the same rules.
 * GSR_E_ARG, before any device work: d_scene NULL with n > 0; GSR_LAYOUT_AOS or an unknown
 * layout; n outside [0, INT32_MAX]; cap outside [GSR_ADAM_OPACITY_MIN, GSR_ADAM_OPACITY_MAX]
 * (or NaN); a pointer that is not 4-byte aligned.  n == 0 is GSR_OK without device work. */
int gsr_scene_reset_opacity(void* d_scene, int layout, int64_t n, float cap, float* d_m_opacity, float* d_v_opacity,
                            void* stream);

/* ---- scene initialisation: a scene block from a point cloud ----
 *
 * The START of the training loop: what structure-from-motion gives, points with colours,
 * becomes a scene block as 3DGS's create_from_pcd builds it — positions the points, SH dc from
 * the colours, identity rotation, one opacity, and every scale the root of the mean squared
 * distance to the point's three nearest neighbours.  That statistic is the only part that is
 * not a fill; it has an entry point of its own and also runs on an existing block's positions.
 * Both calls are context-free.
 *
 * 1. The statistic.  Coordinate c of point i is d_xyz[i * point_stride + c * comp_stride],
 * strides in elements: (3, 1) is an interleaved [n, 3] array, (1, S) is planar with plane
 * stride S (a scene block's own x, y, z arrays with S = the block's stride).
 *
 * The rule.  Everything is float32 with one rounding per operation and no FMA.
 *   - A point is valid when its three coordinates are finite.  Let m be the number of valid
 *     points.
 *   - For valid i and valid j != i (j != i by index, so a coincident point is a neighbour at
 *     distance 0): d2(i,j) = ((dx*dx) + (dy*dy)) + (dz*dz), with dx = x_j - x_i and so on.  The
 *     expression is bitwise symmetric in (i, j).
 *   - Let k = min(3, m - 1), and let b0 <= b1 <= b2 be the k smallest values of d2(i, .),
 *     taken as a multiset.
 *   - d_mean2[i] is ((b0 + b1) + b2) / 3.0f for k = 3; (b0 + b1) / 2.0f for k = 2; b0 for
 *     k = 1; +0 for k = 0.
 *   - A d2 that overflows to +inf is an ordinary value and propagates.
 *   - An invalid point is nobody's neighbour.  Its d_mean2 is +0, and *d_bad (may be NULL; a
 *     device word the caller zeroes) is incremented once per such point.
 * The k smallest VALUES are unique whatever the search order, so the result is exact:
 * reproducible bit for bit, independent of the launch shape, and equal to brute force.  The
 * acceleration structure (a Morton order with 21 bits per axis, leaves of 64 points, two box
 * levels above them) only sets the speed: a box is skipped only when its lower bound, formed by
 * the same expression — per axis e = fmaxf(fmaxf(lo - q, q - hi), 0), then ((ex*ex) + (ey*ey))
 * + (ez*ez) — is strictly greater than the third best so far.  Rounding is monotone, so that
 * float32 bound never exceeds the float32 distance to a point inside the box.
 *
 * Stream-ordered; never allocates and never synchronises; all working memory is d_scratch
 * (gsr_points_knn_scratch_bytes(n) bytes, about 32 n), and nothing is written past
 * scratch_bytes or past d_mean2[n).  No atomics on the output; *d_bad and the bounds inside the
 * scratch are integer atomics.
 * gsr_points_knn_scratch_bytes: >= 0 and non-decreasing in n; negative (GSR_E_ARG) for n
 * outside [0, INT32_MAX].
 * GSR_E_ARG, before any device work: a NULL d_xyz, d_mean2 or d_scratch with n > 0; n outside
 * [0, INT32_MAX]; a stride < 1; point_stride == comp_stride, or strides whose elements overlap
 * for the given n (neither point_stride >= 3 * comp_stride nor comp_stride >= n *
 * point_stride); scratch_bytes below gsr_points_knn_scratch_bytes(n); a pointer that is not
 * 4-byte aligned.  n == 0 is GSR_OK without device work. */
int64_t gsr_points_knn_scratch_bytes(int64_t n);
int gsr_points_knn_dist2(const float* d_xyz, int64_t point_stride, int64_t comp_stride, int64_t n,
                         float* d_mean2 /* n */, uint32_t* d_bad /* or NULL */, void* d_scratch, size_t scratch_bytes,
                         void* stream);

/* 2. The initialiser.  Returns a new scene block as gsr_scene_gather builds it (one hipMalloc;
 * count n, stride rounded up to 64; free with gsr_scene_free; elements in [n, stride)
 * unspecified); narrays is 38, 49 or 59; n == 0 gives a header-only block.  Per Gaussian, in
 * float32 as written:
 *   x, y, z    the point's bits (an invalid point's too: the caller prunes by d_bad / d_mean2)
 *   opacity  = cfg->opacity
 *   scale_c  = fminf(sqrtf(fmaxf(mean2, min_dist2)) * scale_mul, scale_max),  c = 0, 1, 2
 *   rot      = (1, 0, 0, 0)
 *   SH         dc of channel c = (rgb_c - 0.5f) / 0.28209479177387814f (the inverse of the
 *              colour the preprocess forms; d_rgb NULL: 0.5 grey, dc = +0), at sh[c] of a 38- or
 *              49-array block and sh[3 * 0 + c] of a 59-array block; every other SH plane +0;
 *              non-finite colours propagate
 *   a 49-array block adds trbf_center = t_center, trbf_scale = t_scale, motion +0
 * mean2 is gsr_points_knn_dist2 of the points; d_mean2 (may be NULL; n floats) receives it,
 * *d_bad (may be NULL) counts the invalid points.  Colour c of point i is d_rgb[i *
 * rgb_point_stride + c * rgb_comp_stride].
 * The header and the arrays are written on `stream`.  SYNCHRONOUS, like gsr_scene_densify:
 * allocates the block and its own k-NN scratch, waits for `stream`, frees the scratch; called
 * once per run.
 * Returns NULL and sets gsr_last_error on failure.  GSR_E_ARG, before any device work: the
 * cases of gsr_points_knn_dist2 (the rgb strides checked the same way when d_rgb is non-NULL);
 * a bad narrays; a NULL cfg; a NaN field in cfg; opacity outside [GSR_ADAM_OPACITY_MIN,
 * GSR_ADAM_OPACITY_MAX]; min_dist2 < 0; scale_mul <= 0 or not finite; scale_max <= 0; t_scale
 * <= 0 on a 4D block; unknown flag bits. */
typedef struct gsr_init_config {
    float opacity;     /* stored opacity of every Gaussian (3DGS 0.1) */
    float min_dist2;   /* floor on the mean squared distance (3DGS 1e-7) */
    float scale_mul;   /* 1 */
    float scale_max;   /* +inf: off (some trainers cap the initial scale by the scene extent) */
    float t_center;    /* 4D blocks only: stored trbf_center */
    float t_scale;     /* 4D blocks only: stored trbf_scale (> 0) */
    int flags;         /* 0; unknown bits refused */
} gsr_init_config;
void* gsr_scene_from_points(const float* d_xyz, int64_t point_stride, int64_t comp_stride,
                            const float* d_rgb /* or NULL: 0.5 grey */, int64_t rgb_point_stride,
                            int64_t rgb_comp_stride, int64_t n, int narrays, const gsr_init_config* cfg,
                            float* d_mean2 /* n, or NULL */, uint32_t* d_bad /* or NULL */, void* stream);

/* ---- image loss: the step between gsr_render and gsr_render_backward_scene ----
 *
 * The LOSS of render -> LOSS -> gsr_render_backward_scene -> update: the 3DGS training loss
 * of a rendered frame x = d_image against its target y = d_target, and dL/dx in the layout
 * the backward reads.  x and y are 3*W*H floats, planar, in gsr_render's layout (the window
 * below is symmetric, so the bottom-row-first order does not matter).  Context-free,
 * stream-ordered: it never allocates or synchronises; what it needs between its launches
 * lives in the caller's d_scratch.
 *
 *   L = w_l1 * mean|x - y| + w_l2 * mean (x - y)^2 + w_dssim * (1 - mean SSIM(x, y))
 *
 * with every mean over the 3*W*H elements (3DGS: w_l1 0.8, w_l2 0, w_dssim 0.2).  SSIM per
 * channel and pixel, as 3DGS's ssim() computes it with conv2d(padding=5, groups=3):
 *   g_k ~ exp(-(k - 5)^2 / (2 * 1.5^2)), k = 0..10, normalised to sum 1 in double and rounded
 *   to float; the window is g x g, E[.] its weighted sum.  Pixels outside the image count as
 *   0 in all five sums and the window is not renormalised at the border.
 *   mu1 = E[x], mu2 = E[y], s1 = E[x^2] - mu1^2, s2 = E[y^2] - mu2^2, s12 = E[xy] - mu1 mu2
 *   SSIM = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)),
 *   C1 = 1e-4, C2 = 9e-4.
 *
 * d_loss (may be NULL) receives GSR_LOSS_NVALUES floats, OVERWRITTEN: {L, mean|x - y|,
 * mean (x - y)^2 (the MSE: PSNR = -10 log10 of it), mean SSIM}.  They are not scaled by
 * grad_scale.
 * d_grad_image (may be NULL) receives grad_scale * dL/dx, 3*W*H floats, OVERWRITTEN, not
 * accumulated (it is a per-frame input of the backward; grad_scale is 1 / batch size when
 * several frames accumulate into one set of scene gradients).  The L1 term is sign(x - y)
 * with sign(0) = 0; the D-SSIM term is the exact derivative through all five windowed sums (a
 * second windowed sum, of three per-pixel partials).  d_target gets no gradient.  Images
 * with x == y get the gradient 0 exactly.
 *
 * float32 throughout, written with explicit fused multiply-adds; the loss values are summed
 * in double from per-workgroup partial sums, in a fixed order, by a last small launch.  No
 * atomics and no completion counters: results are reproducible bit for bit for given inputs,
 * and a value-only or a gradient-only call gives the bits of the combined call.  Non-finite
 * inputs propagate (gsr_scene_adam_step skips and counts non-finite gradients).
 *
 * gsr_image_loss_scratch_bytes(W, H, want_grad) is what d_scratch must hold for a call with
 * (want_grad != 0) or without a gradient; the value-only size is the smaller, and neither
 * decreases when W*H grows.  The call never touches a byte at or past scratch_bytes; the
 * contents of the scratch between calls are the implementation's and need no initialisation.
 * Negative (GSR_E_ARG) when W or H < 1 or 3*W*H > INT32_MAX.
 *
 * GSR_E_ARG, before any device work: d_image, d_target or cfg NULL; both d_grad_image and
 * d_loss NULL; W or H < 1 or 3*W*H > INT32_MAX; a weight negative or not finite; all three
 * weights 0; grad_scale not finite; unknown flag bits; d_scratch NULL or scratch_bytes below
 * the size of the mode asked for; a pointer that is not 4-byte aligned; d_grad_image equal to
 * d_image or d_target (the gradient launch still reads both).  Any other overlap between the
 * buffers is the caller's business and is not checked. */
typedef struct gsr_loss_config {
    float w_l1;        /* weight of mean |x - y|            (3DGS: 0.8) */
    float w_l2;        /* weight of mean (x - y)^2          (3DGS: 0)   */
    float w_dssim;     /* weight of 1 - mean SSIM(x, y)     (3DGS: 0.2) */
    float grad_scale;  /* d_grad_image = grad_scale * dL/dx (1 / batch size; the loss values are not scaled) */
    int   flags;       /* 0; unknown bits are refused */
} gsr_loss_config;
#define GSR_LOSS_NVALUES 4   /* d_loss: {L, mean |x-y|, mean (x-y)^2, mean SSIM} */

int64_t gsr_image_loss_scratch_bytes(int W, int H, int want_grad);   /* >= 0, or a negative error code */
int gsr_image_loss(const float* d_image, const float* d_target, int W, int H, const gsr_loss_config* cfg,
                   float* d_grad_image /* 3*W*H, OVERWRITTEN, or NULL */,
                   float* d_loss /* GSR_LOSS_NVALUES device floats, OVERWRITTEN, or NULL */,
                   void* d_scratch, int64_t scratch_bytes, void* stream);

/* ---- scene export: a scene block as a 3DGS .ply, the inverse of the loader ----
 *
 * The way out of the loop that gsr_scene_from_points / the loaders open: a block that was
 * trained, pruned or densified on the device becomes a file that gsr_load_ply_device, the
 * reference viewer's loadGaussiansFromPly or any 3DGS tool reads.
 *
 * The row format.  One Gaussian is one row of P = gsr_ply_row_floats(narrays) little-endian
 * floats: 62 for 38- and 59-array blocks, 73 for 49-array (4D) blocks, in the order of the header
 * gsr_synth_write_ply* writes:
 *   x y z | nx ny nz | f_dc_0..2 | f_rest_0..44 | opacity | scale_0..2 | rot_0..3
 *   4D only: | trbf_center | trbf_scale | motion_0..8
 * and the values are the inverse of the loader's store(), per block kind:
 *   x y z, rot_*, trbf_center, motion_*    the stored bits (NaN payloads included)
 *   nx ny nz                               +0
 *   opacity                                gsr_raw_logit(stored)          (gsr_detmath.h)
 *   scale_c, trbf_scale                    gsr_raw_log(stored)
 *   f_dc_c                                 sh[c]
 *   f_rest_j, 38- and 49-array blocks      sh[3 + j] for j < 24, +0 for j = 24..44 (never loaded)
 *   f_rest_j, 59-array blocks              sh[3 (1 + j % 15) + j / 15]    (channel-major again)
 * gsr_raw_log / gsr_raw_logit round alike on the host and the device, so gsr_ply_write_host of a
 * download and gsr_scene_save_ply of the block write the same bytes.  A reload reproduces every
 * copied array bit for bit and the opacity and the scales to the loader's own rounding (the raw
 * functions' error bounds: gsr_detmath.h); a stored opacity of 0 or 1 and a stored scale of 0 or
 * +inf come back as themselves through -inf / +inf, anything the loader cannot have produced
 * (negative, NaN, an opacity above 1) as NaN.
 *
 * Both writers (gsr_scene_save_ply here, gsr_ply_write_host under "host helpers") write the
 * header, then n * P floats (n == 0: the header alone), into a temporary file in the
 * destination's directory and rename it over `path` only on success: on any failure they
 * return GSR_E_IO or GSR_E_HIP, remove the temporary file and leave an existing `path` as it
 * was.  Before any file or device work they refuse with GSR_E_ARG a NULL pointer, a narrays
 * that is no block kind, n outside [0, INT32_MAX] and chunk_rows < 0. */

/* Floats per row of the .ply for a block of `narrays` arrays (62 or 73), or GSR_E_ARG. */
int64_t gsr_ply_row_floats(int narrays);
/* Rows [first, first + count) of the block in the row format, row `first` at d_rows[0]: count *
 * P device floats, and nothing past them is written.  Stream-ordered: no allocation, no wait;
 * (layout, n) are trusted as gsr_scene_adam_step trusts them.  Only [0, n) of an array is read.
 * The stores are 16 B wide when d_rows is 16-B aligned (any hipMalloc is), 4 B otherwise.
 * GSR_E_ARG: the AoS layout or an unknown one, first < 0, count < 0, first + count > n, n outside
 * [0, INT32_MAX], a NULL pointer with count > 0, a pointer off a 4-byte boundary.  count == 0
 * is GSR_OK without device work. */
int gsr_scene_pack_rows(const void* d_scene, int layout, int64_t n, int64_t first, int64_t count,
                        float* d_rows, void* stream);
/* The whole block into the file `path`.  The block's header is checked against (narrays, n) as
 * gsr_scene_copy does (read synchronously); the block itself is only read.  Chunks of
 * chunk_rows rows (0: the default, 65,536) are packed on `stream` into one of two device
 * staging buffers and copied from there into one of two pinned host buffers, and chunk k - 1
 * goes to the file while chunk k is in flight, so a save is bound by the disk.  SYNCHRONOUS on
 * `stream`: work queued on it before the call (an Adam step) is in the file, and the call
 * allocates and frees its four buffers (2 * chunk_rows * P * 4 bytes of each kind). */
int gsr_scene_save_ply(const void* d_scene, int narrays, int64_t n, const char* path,
                       int64_t chunk_rows, void* stream);

/* ---------------------------------------------------------------- host helpers */

/* PLY reader with the semantics of loadGaussianCudaFromPly (misc.cu:13-134 +
 * storeGaussianFromProperty gaussians.cpp:17-30), host side only.  Call with
 * host_soa == NULL to get the count; then with a buffer of 38*n floats. */
int gsr_ply_read_host(const char* path, float* host_soa, int64_t capacity, int64_t* n_out);
/* Same with flags (GSR_PLY_TYPED, GSR_PLY_SH3) and narrays = 38, 49 (4D arrays
 * filled when present; defaults trbf_center 0, trbf_scale 1, motion 0) or 59
 * (with GSR_PLY_SH3); *is_4d (if non-NULL) reports whether the file has the 4D
 * properties. */
int gsr_ply_read_host_ex(const char* path, float* host_soa, int narrays, int64_t capacity, int64_t* n_out,
                         int flags, int* is_4d);

/* PLY writer, the inverse of gsr_ply_read_host_ex ("scene export" above has the row format and
 * what both writers share): host_soa holds narrays (38, 49 or 59) arrays of n floats as
 * gsr_scene_download gives them, activated.  Byte-identical to gsr_scene_save_ply of a block
 * with the same values. */
int gsr_ply_write_host(const char* path, const float* host_soa, int narrays, int64_t n);
/* gsr_raw_log (kind 0) or gsr_raw_logit (kind 1) of gsr_detmath.h over n host floats: the raw
 * values the writers store for a scale and an opacity.  GSR_E_ARG: a NULL pointer, n < 0,
 * another kind. */
int gsr_raw_probe(const float* host_in, int n, int kind, float* host_out);

/* Seeded synthetic scene: writes a standard 62-property
 * binary_little_endian 3DGS .ply, or fills raw (pre-activation) property
 * values.  Same generator, same values, for a given (n, seed). */
int gsr_synth_write_ply(const char* path, int64_t n, uint64_t seed);
/* Config 5 4D synthetic scene: the 62 properties plus trbf_center U(0,1),
 * trbf_scale U(-3.5,-2) (log), motion_0..8 N(0, .5 | .2 | .1). */
int gsr_synth_write_ply4d(const char* path, int64_t n, uint64_t seed);

/* Camera (camera.cpp): Camera() ctor 8-13, updateCameraMatrices 36-57,
 * updateFrustumPlanes 59-121, zoom 123-128, orbit 130-158. */
void gsr_camera_default(gsr_camera* cam);
void gsr_camera_update(gsr_camera* cam);
void gsr_camera_update_frustum(gsr_camera* cam);
void gsr_camera_zoom(gsr_camera* cam, float delta);
void gsr_camera_orbit(gsr_camera* cam, float azimuth_deg, float elevation_deg);
/* fx, fy exactly as render.cu:620-621 (tanf computed correctly rounded). */
void gsr_camera_intrinsics(const gsr_camera* cam, float* fx, float* fy);

/* Device self-test used by the parity tests: for each (x, y) pair of host_in
 * (2n floats) evaluates on the GPU {gsr_expf(x), gsr_sinf(x), gsr_cosf(x),
 * gsr_atan2f(x, y), sqrtf(x), x / y, roundf(x), bits(gsr_f2i_sat(1000x)),
 * gsr_blend_expf(x)} into host_out (9n floats), so the CPU twins can be compared
 * bit for bit. */
int gsr_math_probe(const float* host_in, int n, float* host_out);
/* Exhaustive device checks of the blend's exp, over every float x in [x_lo, x_hi):
 * *violations = the number of x with gsr_blend_expf(x) > gsr_blend_expf(next x)
 * (0: the exact exp is monotone, so the alpha test is a threshold on -md2/2);
 * *err_all / *err_big = the largest |fast exp / gsr_blend_expf - 1|
 * (GSR_TUNE_BLEND_EXP 1) over the range / over x >= x_big (rounded up).
 * violations points at ONE int64 (the round-3 signature, unchanged). */
int gsr_exp_probe(float x_lo, float x_hi, float x_big, int64_t* violations, float* err_all, float* err_big);
/* gsr_exp_probe plus *packed_mismatches = the number of x in [-2e7, 5] (and of -x
 * there) where the packed compositing loop's exp differs from gsr_blend_expf
 * (0: the packed and scalar exps agree bit for bit).  Each pointer names one value. */
int gsr_exp_probe2(float x_lo, float x_hi, float x_big, int64_t* violations, int64_t* packed_mismatches,
                   float* err_all, float* err_big);
/* gsr_alpha_take_min_x (gsr_detmath.h) evaluated on the device for n opacities. */
int gsr_alpha_cut_probe(const float* host_op, int n, float* host_out);

const char* gsr_last_error(void);
const char* gsr_version(void);
/* 1 if a HIP device is usable, else 0 (never aborts). */
int gsr_device_available(void);

#ifdef __cplusplus
}  /* extern "C" */

#include <string>
/* misc.cuh:4 — C++ linkage, same mangled name as the reference's loader. */
gsr_gaussian* loadGaussianCudaFromPly(const std::string& filename, int* out_numGaussians);
#endif

#endif /* GSR_H */

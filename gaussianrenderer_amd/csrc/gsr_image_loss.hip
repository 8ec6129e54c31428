// gsr_image_loss.hip — the loss between render and backward (include/gsr.h "image loss"):
// (1 - lambda) L1 + lambda (1 - SSIM) of a frame against its target, the four loss values and
// dL/d image in the layout gsr_render_backward_scene reads.  Two tiled launches and a small
// one; the window sums never leave the LDS.
#include "gsr_device.h"

namespace gsr {

namespace {

// The 11-tap window of 3DGS's ssim(): exp(-(k - 5)^2 / (2 * 1.5^2)), k = 0..10, normalised in
// double and rounded to float.  Indexed by a compile-time k in unrolled loops only, so each
// weight is an instruction literal.
constexpr int kLossR = 5;                    // window radius
constexpr int kLossTaps = 2 * kLossR + 1;
constexpr float kLossG[kLossTaps] = {1.028380124e-03f, 7.598758209e-03f, 3.600077331e-02f, 1.093606874e-01f,
                                     2.130055428e-01f, 2.660117149e-01f, 2.130055428e-01f, 1.093606874e-01f,
                                     3.600077331e-02f, 7.598758209e-03f, 1.028380124e-03f};
constexpr float kLossC1 = 1e-4f, kLossC2 = 9e-4f;

// One workgroup of 256 threads owns a 16 x 16 tile of one channel at a time, thread (tx, ty)
// its pixel, and walks tiles t = blockIdx.x, + gridDim.x, ... (at most kLossMaxGroups
// workgroups, so the loss partials in scratch have a fixed size).  Per tile:
//   stage   the tile and its 5-pixel halo, 26 x 26, zero outside the image, into the LDS;
//   rows    the horizontal 11-tap sums for the 26 rows x 16 columns (416 items over 256
//           threads), back to the LDS;
//   columns each thread's vertical 11-tap sum of its column.
// The VALU sets the pace (hundreds of instructions per pixel against 20 bytes of traffic), so
// the sums run two to an instruction where they pair up: x and y sit side by side in the LDS
// as one float2, and {E[x], E[y]} and {E[x^2], E[y^2]} are each one packed multiply-add per
// tap (v_pk_fma_f32; the backward pairs two of its three maps the same way).
// LDS banking (a wave's LDS access is served in groups of 32 lanes = two 16-wide rows of items
// here; 32 banks for 4-byte accesses, 64 for 8-byte ones): the staged rows are
// kLossStageStride = 48 elements apart, so two consecutive rows' 16 elements fall in disjoint
// halves of the banks for every tap; the row sums are stored 16 elements a row, so the column
// pass reads 32 consecutive elements.
constexpr int kLossTile = 16;
constexpr int kLossThreads = kLossTile * kLossTile;
constexpr int kLossSpan = kLossTile + 2 * kLossR;   // 26
constexpr int kLossStageStride = 48;
constexpr int kLossRowItems = kLossSpan * kLossTile;   // 416

typedef float loss_f2 __attribute__((ext_vector_type(2)));

// a * b + c per lane, fused (the build never contracts on its own)
__device__ __forceinline__ loss_f2 loss_fma2(loss_f2 a, loss_f2 b, loss_f2 c) {
    return __builtin_elementwise_fma(a, b, c);
}

struct LossTile {
    int ch, x0, y0;   // channel, first pixel
};

__device__ __forceinline__ LossTile loss_tile(int t, int tiles_x, int tiles_per_ch) {
    const int ch = t / tiles_per_ch, r = t - ch * tiles_per_ch;
    const int ty = r / tiles_x;
    return LossTile{ch, (r - ty * tiles_x) * kLossTile, ty * kLossTile};
}

// sa[r][c] = a[(y0 - 5 + r) * W + x0 - 5 + c] and sbc[r][c] = {b[..], c[..]}, 0 outside the
// image; sa and a may be null (the forward stages a pair only).
__device__ __forceinline__ void loss_stage(const float* __restrict__ a, const float* __restrict__ b,
                                           const float* __restrict__ c, int W, int H, int x0, int y0,
                                           float (*sa)[kLossStageStride], loss_f2 (*sbc)[kLossStageStride]) {
    for (int i = threadIdx.x; i < kLossSpan * kLossSpan; i += kLossThreads) {
        const int r = i / kLossSpan, col = i - r * kLossSpan;
        const int gx = x0 - kLossR + col, gy = y0 - kLossR + r;
        const bool in = gx >= 0 && gx < W && gy >= 0 && gy < H;
        const int at = in ? gy * W + gx : 0;   // < W * H <= INT32_MAX / 3
        loss_f2 v;
        v.x = in ? b[at] : 0.0f;
        v.y = in ? c[at] : 0.0f;
        sbc[r][col] = v;
        if (sa) sa[r][col] = in ? a[at] : 0.0f;
    }
}

// A fixed-order sum over the workgroup: a butterfly inside each wave, then the four waves'
// totals in wave order.  `part` holds 4 floats; contains one barrier.  The result is valid
// in thread 0.
__device__ __forceinline__ float loss_block_sum(float v, float* part) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if (lane_id() == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((part[0] + part[1]) + part[2]) + part[3];
}

// Forward.  x, y: the 3 planes of W * H.  GRAD: write the three per-pixel partials of SSIM
// with respect to the windowed means E[x], E[x^2], E[xy] to part (3 maps of 3 * W * H; the
// first already carries the -2 mu1 and -mu2 terms of the other two).  VALUE: write this
// workgroup's sums of |x - y|, (x - y)^2 and SSIM to slots[3 * blockIdx.x ..].
//
// SSIM is formed as (A1 / B1) * (A2 / B2) and its partials from those two quotients: for
// x == y the numerators equal the denominators bit for bit, the quotients are exactly 1 and
// the three partials cancel exactly in the backward's combination, so equal images get the
// gradient 0 and not rounding noise.
template <bool GRAD, bool VALUE>
__global__ __launch_bounds__(kLossThreads) void k_image_loss_forward(const float* __restrict__ x,
                                                                     const float* __restrict__ y, int W, int H,
                                                                     int tiles_x, int tiles_per_ch, int ntiles,
                                                                     float* __restrict__ part,
                                                                     float* __restrict__ slots) {
    __shared__ loss_f2 sxy[kLossSpan][kLossStageStride];                      // {x, y}
    __shared__ loss_f2 rows_m[kLossSpan][kLossTile], rows_e[kLossSpan][kLossTile];   // {E x, E y}, {E xx, E yy}
    __shared__ float rows_xy[kLossSpan][kLossTile];
    __shared__ float red[3][4];
    const int tx = threadIdx.x & (kLossTile - 1), ty = threadIdx.x >> 4;
    const int64_t plane = (int64_t)W * H;
    float sum_abs = 0.0f, sum_sq = 0.0f, sum_ssim = 0.0f;

    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const LossTile tl = loss_tile(t, tiles_x, tiles_per_ch);
        loss_stage(nullptr, x + tl.ch * plane, y + tl.ch * plane, W, H, tl.x0, tl.y0, nullptr, sxy);
        __syncthreads();

        for (int i = threadIdx.x; i < kLossRowItems; i += kLossThreads) {
            const int r = i >> 4, c = i & (kLossTile - 1);
            loss_f2 m = {0.0f, 0.0f}, e = {0.0f, 0.0f};
            float exy = 0.0f;
#pragma unroll
            for (int k = 0; k < kLossTaps; k++) {
                const loss_f2 ab = sxy[r][c + k];
                const loss_f2 gab = kLossG[k] * ab;
                m += gab;
                e = loss_fma2(gab, ab, e);
                exy = fmaf(gab.x, ab.y, exy);
            }
            rows_m[r][c] = m;
            rows_e[r][c] = e;
            rows_xy[r][c] = exy;
        }
        const loss_f2 cxy = sxy[ty + kLossR][tx + kLossR];
        __syncthreads();

        loss_f2 m = {0.0f, 0.0f}, e = {0.0f, 0.0f};
        float e12 = 0.0f;
#pragma unroll
        for (int k = 0; k < kLossTaps; k++) {
            const loss_f2 g2 = {kLossG[k], kLossG[k]};
            m = loss_fma2(g2, rows_m[ty + k][tx], m);
            e = loss_fma2(g2, rows_e[ty + k][tx], e);
            e12 = fmaf(kLossG[k], rows_xy[ty + k][tx], e12);
        }
        const float m1 = m.x, m2 = m.y, e11 = e.x, e22 = e.y;
        const int px = tl.x0 + tx, py = tl.y0 + ty;
        if (px < W && py < H) {
            const float s1 = e11 - m1 * m1, s2 = e22 - m2 * m2, s12 = e12 - m1 * m2;
            const float a1 = (2.0f * m1) * m2 + kLossC1, a2 = 2.0f * s12 + kLossC2;
            const float b1 = (m1 * m1 + m2 * m2) + kLossC1, b2 = (s1 + s2) + kLossC2;
            const float ra = a1 / b1, rb = a2 / b2;
            const float ssim = ra * rb;
            if (VALUE) {
                const float d = cxy.x - cxy.y;
                sum_abs += fabsf(d);
                sum_sq = fmaf(d, d, sum_sq);
                sum_ssim += ssim;
            }
            if (GRAD) {
                const float ib1 = 1.0f / b1, ib2 = 1.0f / b2;
                const float p2 = -(ssim * ib2);                 // d SSIM / d sigma1^2
                const float p3 = (2.0f * ra) * ib2;             // d SSIM / d sigma12
                const float direct = (2.0f * (m2 * rb - m1 * ssim)) * ib1;
                const float p1 = (direct - (2.0f * m1) * p2) - m2 * p3;   // d SSIM / d E[x]
                const int64_t at = tl.ch * plane + (py * W + px);
                part[at] = p1;
                part[3 * plane + at] = p2;
                part[6 * plane + at] = p3;
            }
        }
        // the next tile's staging writes sxy (no longer read) and meets a barrier before its
        // row pass writes the row sums
    }
    if (VALUE) {
        const float a = loss_block_sum(sum_abs, red[0]);
        const float q = loss_block_sum(sum_sq, red[1]);
        const float s = loss_block_sum(sum_ssim, red[2]);
        if (threadIdx.x == 0) {
            slots[3 * blockIdx.x + 0] = a;
            slots[3 * blockIdx.x + 1] = q;
            slots[3 * blockIdx.x + 2] = s;
        }
    }
}

// The four loss values from the ngroups slot triples: thread t sums slots t, t + 256, ... in
// double, then a fixed tree over the workgroup.  One workgroup.
__global__ __launch_bounds__(kLossThreads) void k_image_loss_values(const float* __restrict__ slots, int ngroups,
                                                                    double count, double w_l1, double w_l2,
                                                                    double w_dssim, float* __restrict__ out) {
    __shared__ double acc[3][kLossThreads];
    double a = 0.0, q = 0.0, s = 0.0;
    for (int g = threadIdx.x; g < ngroups; g += kLossThreads) {
        a += (double)slots[3 * g + 0];
        q += (double)slots[3 * g + 1];
        s += (double)slots[3 * g + 2];
    }
    acc[0][threadIdx.x] = a;
    acc[1][threadIdx.x] = q;
    acc[2][threadIdx.x] = s;
    __syncthreads();
    for (int h = kLossThreads / 2; h >= 1; h >>= 1) {
        if ((int)threadIdx.x < h) {
#pragma unroll
            for (int k = 0; k < 3; k++) acc[k][threadIdx.x] += acc[k][threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double l1 = acc[0][0] / count, l2 = acc[1][0] / count, ssim = acc[2][0] / count;
        out[0] = (float)(w_l1 * l1 + w_l2 * l2 + w_dssim * (1.0 - ssim));
        out[1] = (float)l1;
        out[2] = (float)l2;
        out[3] = (float)ssim;
    }
}

// Backward.  The same tiling over the three partial maps (zero outside the image):
//   grad = c_ssim * (W*p1 + 2 x W*p2 + y W*p3) + c_l1 * sign(x - y) + c_l2 * (x - y)
// with W* the 11 x 11 window and c_* = grad_scale * weight / (3 W H) (c_ssim negative, c_l2
// doubled), formed by the host in double.
__global__ __launch_bounds__(kLossThreads) void k_image_loss_backward(const float* __restrict__ x,
                                                                      const float* __restrict__ y, int W, int H,
                                                                      int tiles_x, int tiles_per_ch, int ntiles,
                                                                      const float* __restrict__ part, float c_l1,
                                                                      float c_l2, float c_ssim,
                                                                      float* __restrict__ grad) {
    __shared__ float sp1[kLossSpan][kLossStageStride];
    __shared__ loss_f2 sp23[kLossSpan][kLossStageStride];
    __shared__ float rows1[kLossSpan][kLossTile];
    __shared__ loss_f2 rows23[kLossSpan][kLossTile];
    const int tx = threadIdx.x & (kLossTile - 1), ty = threadIdx.x >> 4;
    const int64_t plane = (int64_t)W * H;

    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const LossTile tl = loss_tile(t, tiles_x, tiles_per_ch);
        const int px = tl.x0 + tx, py = tl.y0 + ty;
        const bool in = px < W && py < H;
        const int64_t at = tl.ch * plane + (in ? py * W + px : 0);
        // the pixel's own x and y: in flight while the window sums run
        const float cx = in ? x[at] : 0.0f, cy = in ? y[at] : 0.0f;
        const float* p1 = part + tl.ch * plane;
        loss_stage(p1, p1 + 3 * plane, p1 + 6 * plane, W, H, tl.x0, tl.y0, sp1, sp23);
        __syncthreads();

        for (int i = threadIdx.x; i < kLossRowItems; i += kLossThreads) {
            const int r = i >> 4, c = i & (kLossTile - 1);
            float h1 = 0.0f;
            loss_f2 h23 = {0.0f, 0.0f};
#pragma unroll
            for (int k = 0; k < kLossTaps; k++) {
                const loss_f2 g2 = {kLossG[k], kLossG[k]};
                h1 = fmaf(kLossG[k], sp1[r][c + k], h1);
                h23 = loss_fma2(g2, sp23[r][c + k], h23);
            }
            rows1[r][c] = h1;
            rows23[r][c] = h23;
        }
        __syncthreads();

        float w1 = 0.0f;
        loss_f2 w23 = {0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < kLossTaps; k++) {
            const loss_f2 g2 = {kLossG[k], kLossG[k]};
            w1 = fmaf(kLossG[k], rows1[ty + k][tx], w1);
            w23 = loss_fma2(g2, rows23[ty + k][tx], w23);
        }
        const float w2 = w23.x, w3 = w23.y;
        if (in) {
            const float d = cx - cy;
            const float sign = (float)(d > 0.0f) - (float)(d < 0.0f);   // sign(0) = 0
            // two rounded products, not an fmaf: for x == y they are R and -R and cancel
            const float ds = w1 + ((2.0f * cx) * w2 + cy * w3);
            grad[at] = fmaf(c_ssim, ds, fmaf(c_l2, d, c_l1 * sign));
        }
    }
}

}  // namespace

hipError_t launch_image_loss(const float* x, const float* y, int W, int H, const LossLaunch& L, float* grad,
                             float* loss, float* scratch, hipStream_t s) {
    const int tiles_x = grid_for(W, kLossTile), tiles_y = grid_for(H, kLossTile);
    const int64_t ntiles64 = 3 * (int64_t)tiles_x * tiles_y;   // <= 3 W H <= INT32_MAX
    const int ntiles = (int)ntiles64, tiles_per_ch = tiles_x * tiles_y;
    const int groups = std::min(ntiles, kLossMaxGroups);
    float* slots = scratch;
    float* part = scratch + kLossSlotFloats;   // only touched (and only there) with a gradient
    with_bool(grad != nullptr, [&](auto g) {
        with_bool(loss != nullptr, [&](auto v) {
            hipLaunchKernelGGL((k_image_loss_forward<decltype(g)::value, decltype(v)::value>), dim3(groups),
                               dim3(kLossThreads), 0, s, x, y, W, H, tiles_x, tiles_per_ch, ntiles, part, slots);
            return 0;
        });
        return 0;
    });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (loss) {
        hipLaunchKernelGGL(k_image_loss_values, dim3(1), dim3(kLossThreads), 0, s, slots, groups,
                           3.0 * (double)W * (double)H, L.w_l1, L.w_l2, L.w_dssim, loss);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (grad) {
        hipLaunchKernelGGL(k_image_loss_backward, dim3(groups), dim3(kLossThreads), 0, s, x, y, W, H, tiles_x,
                           tiles_per_ch, ntiles, part, L.c_l1, L.c_l2, L.c_ssim, grad);
        e = hipGetLastError();
    }
    return e;
}

}  // namespace gsr

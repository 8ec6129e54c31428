// gsr_project.hip — backward pass of the preprocess's projection (gsr_project_backward,
// include/gsr.h): the gradients gsr_render_backward leaves at each Gaussian's splat record
// (colour, opacity, 2D conic, 2D centre) carried on to the scene arrays (position, opacity,
// scale, rotation, SH, and the temporal arrays of a 4D block).
//
// The forward half restates preprocess_camera (gsr_kernels.hip) through the code both share
// (gsr_preprocess_device.h), with the same operation order and no FMA contraction, so the
// three tests that decide whether a record exists fall as they fell in the frame.  The
// screen-extent reject and the 4D temporal cull are not re-evaluated: a Gaussian they drop
// never composites and arrives with zero upstream, which is tested first.
//
// The backward half is hand-derived (the chain is written out beside each step) and checked
// against torch.autograd of a float64 restatement (tests/_project_ref.py).  One thread owns
// one Gaussian and adds to each output plane with a plain load-add-store: no atomics, the
// results are reproducible bit for bit.
#include "gsr.h"
#include "gsr_device.h"
#include "gsr_preprocess_device.h"

namespace gsr {

namespace {

// Basis function k of the real spherical harmonics the preprocess evaluates (render.cu:500-534
// for bands 0..2; band 3 as the 3DGS training code), B, and its gradient with respect to the
// direction, dB: colour channel c is sum_k B_k sh[3 k + c] + 0.5.
struct ShDir {
    float x, y, z, xx, yy, zz, xy, yz, xz;
};

__device__ __forceinline__ void sh_basis(int k, const ShDir& d, float& B, float* dB) {
    const float C2_0 = 1.0925484305920792f, C2_1 = -1.0925484305920792f, C2_2 = 0.31539156525252005f,
                C2_3 = -1.0925484305920792f, C2_4 = 0.5462742152960396f;
    const float C3_0 = -0.5900435899266435f, C3_1 = 2.890611442640554f, C3_2 = -0.4570457994644658f,
                C3_3 = 0.3731763325901154f, C3_4 = -0.4570457994644658f, C3_5 = 1.445305721320277f,
                C3_6 = -0.5900435899266435f;
    const float x = d.x, y = d.y, z = d.z, xx = d.xx, yy = d.yy, zz = d.zz, xy = d.xy, yz = d.yz, xz = d.xz;
    switch (k) {
    case 0: B = kShC0; dB[0] = 0.0f; dB[1] = 0.0f; dB[2] = 0.0f; break;
    case 1: B = -kShC1 * y; dB[0] = 0.0f; dB[1] = -kShC1; dB[2] = 0.0f; break;
    case 2: B = kShC1 * z; dB[0] = 0.0f; dB[1] = 0.0f; dB[2] = kShC1; break;
    case 3: B = -kShC1 * x; dB[0] = -kShC1; dB[1] = 0.0f; dB[2] = 0.0f; break;
    case 4: B = C2_0 * xy; dB[0] = C2_0 * y; dB[1] = C2_0 * x; dB[2] = 0.0f; break;
    case 5: B = C2_1 * yz; dB[0] = 0.0f; dB[1] = C2_1 * z; dB[2] = C2_1 * y; break;
    case 6:
        B = C2_2 * (2.0f * zz - xx - yy);
        dB[0] = C2_2 * (-2.0f * x); dB[1] = C2_2 * (-2.0f * y); dB[2] = C2_2 * (4.0f * z);
        break;
    case 7: B = C2_3 * xz; dB[0] = C2_3 * z; dB[1] = 0.0f; dB[2] = C2_3 * x; break;
    case 8: B = C2_4 * (xx - yy); dB[0] = C2_4 * (2.0f * x); dB[1] = C2_4 * (-2.0f * y); dB[2] = 0.0f; break;
    case 9:
        B = C3_0 * y * (3.0f * xx - yy);
        dB[0] = C3_0 * (6.0f * xy); dB[1] = C3_0 * (3.0f * xx - 3.0f * yy); dB[2] = 0.0f;
        break;
    case 10: B = C3_1 * xy * z; dB[0] = C3_1 * yz; dB[1] = C3_1 * xz; dB[2] = C3_1 * xy; break;
    case 11:
        B = C3_2 * y * (4.0f * zz - xx - yy);
        dB[0] = C3_2 * (-2.0f * xy); dB[1] = C3_2 * (4.0f * zz - xx - 3.0f * yy); dB[2] = C3_2 * (8.0f * yz);
        break;
    case 12:
        B = C3_3 * z * (2.0f * zz - 3.0f * xx - 3.0f * yy);
        dB[0] = C3_3 * (-6.0f * xz); dB[1] = C3_3 * (-6.0f * yz); dB[2] = C3_3 * (6.0f * zz - 3.0f * xx - 3.0f * yy);
        break;
    case 13:
        B = C3_4 * x * (4.0f * zz - xx - yy);
        dB[0] = C3_4 * (4.0f * zz - 3.0f * xx - yy); dB[1] = C3_4 * (-2.0f * xy); dB[2] = C3_4 * (8.0f * xz);
        break;
    case 14:
        B = C3_5 * z * (xx - yy);
        dB[0] = C3_5 * (2.0f * xz); dB[1] = C3_5 * (-2.0f * yz); dB[2] = C3_5 * (xx - yy);
        break;
    default:
        B = C3_6 * x * (xx - 3.0f * yy);
        dB[0] = C3_6 * (3.0f * xx - 3.0f * yy); dB[1] = C3_6 * (-6.0f * xy); dB[2] = 0.0f;
        break;
    }
}

// Plane c of an n-strided gradient array for the workgroup's Gaussians: p + c n + the
// workgroup's first index is uniform, the lane adds its own index (as SoaWg).
struct PlanesWg {
    int64_t n, i0;
    uint32_t lane;
    __device__ __forceinline__ float in(const float* p, int c) const {
        return p ? (p + (c * n + i0))[lane] : 0.0f;
    }
    __device__ __forceinline__ void add(float* p, int c, float v) const {
        float* q = p + (c * n + i0);
        q[lane] = q[lane] + v;
    }
};

// One Gaussian per lane, 256 per workgroup.  T4D: a 49-array block at time tnow; SH3: a
// 59-array block (bands 0..3, clamped at 0 only).  DZ (gsr_project_backward_aux): in_z holds
// an eleventh upstream entry, dL/d(-Z); without it the kernel is the ten-entry one, operation
// for operation (in_z, last, is not read).
template <bool T4D, bool SH3, bool DZ>
__global__ __launch_bounds__(256) void k_project_backward(const float* __restrict__ arr, int64_t stride, int64_t n,
                                                          Frame fr, float tnow, const gsr_record_grads in,
                                                          const gsr_scene_grads out, const float* __restrict__ in_z) {
    const int64_t i0 = (int64_t)blockIdx.x * 256;
    if (i0 + threadIdx.x >= n) return;
    const PlanesWg G{n, i0, threadIdx.x};

    // ---- upstream: the ten record gradients (DZ: and dL/d(-Z)); all zero = the frame never
    // composited it ----
    float g_col[3], g_con[4], g_cen[2];
#pragma unroll
    for (int c = 0; c < 3; c++) g_col[c] = G.in(in.d_color, c);
    const float g_op = G.in(in.d_opacity, 0);
#pragma unroll
    for (int c = 0; c < 4; c++) g_con[c] = G.in(in.d_conic, c);
#pragma unroll
    for (int c = 0; c < 2; c++) g_cen[c] = G.in(in.d_center, c);
    const float g_z = DZ ? G.in(in_z, 0) : 0.0f;
    if (g_col[0] == 0.0f && g_col[1] == 0.0f && g_col[2] == 0.0f && g_op == 0.0f && g_con[0] == 0.0f &&
        g_con[1] == 0.0f && g_con[2] == 0.0f && g_con[3] == 0.0f && g_cen[0] == 0.0f && g_cen[1] == 0.0f &&
        (!DZ || g_z == 0.0f))
        return;

    // ---- forward, as preprocess_camera: view, clip, 2D covariance, the three tests ----
    constexpr bool kEarlySH = PreLoads<T4D, SH3>::kEarlySH;
    constexpr int kCoef = SH3 ? 16 : 9;
    const SoaWg A{arr + i0, stride, 4u * threadIdx.x};
    PreLoads<T4D, SH3> L;
    preprocess_load<T4D, SH3>(A, tnow, L);
    const float pos[4] = {L.gx, L.gy, L.gz, 1.0f};
    float view[4], clip[4], ndc[3];
    mv4(fr.V, pos, view);
    if (GSR_VIEW_CULLED(view)) return;
    mv4(fr.P, view, clip);
    ndc[0] = clip[0] / clip[3];
    ndc[1] = clip[1] / clip[3];
    ndc[2] = clip[2] / clip[3];
    if (GSR_CLIP_CULLED(fr, view, ndc)) return;

    const float X = view[0], Y = view[1], Z = view[2];
    const float fx = fr.fx, fy = fr.fy;
    float jac[6], jacT[6];
    jac[0] = fx / Z; jac[1] = 0.0f;
    jac[2] = -fx * X / (Z * Z); jac[3] = 0.0f;
    jac[4] = fy / Z; jac[5] = -fy * Y / (Z * Z);
    jacT[0] = jac[0]; jacT[1] = jac[3]; jacT[2] = jac[1];
    jacT[3] = jac[4]; jacT[4] = jac[2]; jacT[5] = jac[5];
    float tmp[9], covc[9], JS[6], M[4];
    preprocess_cov3d(L.q_in, L.s_in, covc);
    mm3(fr.Rc, covc, tmp);
    mm3(tmp, fr.RcT, covc);              // Sigma_c = Rc Sigma Rc^T
    gemm<2, 3, 3>(jac, covc, JS);        // J Sigma_c
    gemm<2, 2, 3>(JS, jacT, M);          // T = J Sigma_c J^T
    const int W = fr.W, H = fr.H;
    const float D[4] = {(W * 0.5f) * (W * 0.5f), (W * 0.5f) * (H * 0.5f), (H * 0.5f) * (W * 0.5f),
                        (H * 0.5f) * (H * 0.5f)};
#pragma unroll
    for (int k = 0; k < 4; k++) M[k] = D[k] * M[k];
    const float det = M[0] * M[3] - M[1] * M[2];
    if (GSR_DET_CULLED(det)) return;
    const float invDet = 1.0f / det;
    const float ka = M[3] * invDet, kb = -M[1] * invDet, kc = -M[2] * invDet, ke = M[0] * invDet;

    // ---- conic: K = [[a, b], [c, e]] = M^-1, dL/dM = -K^T G K^T, dL/dT = D o dL/dM ----
    float dT[4];
    {
        const float q00 = g_con[0] * ka + g_con[1] * kb, q01 = g_con[0] * kc + g_con[1] * ke;   // G K^T
        const float q10 = g_con[2] * ka + g_con[3] * kb, q11 = g_con[2] * kc + g_con[3] * ke;
        dT[0] = D[0] * -(ka * q00 + kc * q10);
        dT[1] = D[1] * -(ka * q01 + kc * q11);
        dT[2] = D[2] * -(kb * q00 + ke * q10);
        dT[3] = D[3] * -(kb * q01 + ke * q11);
    }
    // dL/dJ = dT (J Sigma_c^T) + dT^T (J Sigma_c); J depends on the view position through
    // J00 = fx / Z, J02 = -fx X / Z^2, J11 = fy / Z, J12 = -fy Y / Z^2
    float d_view[4];
    {
        float covcT[9], JSt[6], dJ[6];
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int s = 0; s < 3; s++) covcT[r * 3 + s] = covc[s * 3 + r];
        gemm<2, 3, 3>(jac, covcT, JSt);
#pragma unroll
        for (int j = 0; j < 3; j++) {
            dJ[j] = (dT[0] * JSt[j] + dT[1] * JSt[3 + j]) + (dT[0] * JS[j] + dT[2] * JS[3 + j]);
            dJ[3 + j] = (dT[2] * JSt[j] + dT[3] * JSt[3 + j]) + (dT[1] * JS[j] + dT[3] * JS[3 + j]);
        }
        const float iz = 1.0f / Z, iz2 = iz * iz, iz3 = iz2 * iz;
        d_view[0] = dJ[2] * (-fx * iz2);
        d_view[1] = dJ[5] * (-fy * iz2);
        d_view[2] = dJ[0] * (-fx * iz2) + dJ[2] * (2.0f * fx * X * iz3) + dJ[4] * (-fy * iz2) +
                    dJ[5] * (2.0f * fy * Y * iz3);
        d_view[3] = 0.0f;
    }
    // ---- centre = ((ndc + 1) W/2, (ndc + 1) H/2), the rounding differentiated as identity ----
    {
        const float dnx = g_cen[0] * (W * 0.5f), dny = g_cen[1] * (H * 0.5f);
        const float iw = 1.0f / clip[3];
        const float d_clip[4] = {dnx * iw, dny * iw, 0.0f, -(dnx * ndc[0] + dny * ndc[1]) * iw};
#pragma unroll
        for (int j = 0; j < 4; j++) d_view[j] += fr.P[j] * d_clip[0] + fr.P[4 + j] * d_clip[1] + fr.P[12 + j] * d_clip[3];
    }
    float d_pos[3];
#pragma unroll
    for (int j = 0; j < 3; j++)
        d_pos[j] = fr.V[j] * d_view[0] + fr.V[4 + j] * d_view[1] + fr.V[8 + j] * d_view[2] + fr.V[12 + j] * d_view[3];
    if (DZ) {   // Z = (V [p, 1])_z: dL/dp += -V[2][.] dL/d(-Z)
#pragma unroll
        for (int j = 0; j < 3; j++) d_pos[j] += -fr.V[8 + j] * g_z;
    }

    // ---- covariance: dL/dSigma_c = J^T dT J, dL/dSigma = Rc^T (.) Rc, N = R S, Sigma = N N^T,
    // dL/dN = (G + G^T) N; then the scales, the rotation matrix and the quaternion ----
    if (out.d_scale || out.d_rot) {
        float E[6], dS[9];
        gemm<2, 3, 2>(dT, jac, E);
        gemm<3, 3, 2>(jacT, E, tmp);
        mm3(fr.RcT, tmp, dS);
        mm3(dS, fr.Rc, tmp);
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int s = 0; s < 3; s++) dS[r * 3 + s] = tmp[r * 3 + s] + tmp[s * 3 + r];
        const float qn = sqrtf(L.q_in[1] * L.q_in[1] + L.q_in[2] * L.q_in[2] + L.q_in[3] * L.q_in[3] +
                               L.q_in[0] * L.q_in[0]);
        const float iqn = 1.0f / qn;
        const float qw = L.q_in[0] * iqn, qx = L.q_in[1] * iqn, qy = L.q_in[2] * iqn, qz = L.q_in[3] * iqn;
        float R[9], N[9], dN[9];
        R[0] = 1 - 2 * qy * qy - 2 * qz * qz; R[1] = 2 * qx * qy - 2 * qw * qz;     R[2] = 2 * qx * qz + 2 * qw * qy;
        R[3] = 2 * qx * qy + 2 * qw * qz;     R[4] = 1 - 2 * qx * qx - 2 * qz * qz; R[5] = 2 * qy * qz - 2 * qw * qx;
        R[6] = 2 * qx * qz - 2 * qw * qy;     R[7] = 2 * qy * qz + 2 * qw * qx;     R[8] = 1 - 2 * qx * qx - 2 * qy * qy;
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int s = 0; s < 3; s++) N[r * 3 + s] = R[r * 3 + s] * L.s_in[s];
        mm3(dS, N, dN);
        if (out.d_scale) {
#pragma unroll
            for (int s = 0; s < 3; s++)
                G.add(out.d_scale, s, dN[s] * R[s] + dN[3 + s] * R[3 + s] + dN[6 + s] * R[6 + s]);
        }
        if (out.d_rot) {
            float dR[9];
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int s = 0; s < 3; s++) dR[r * 3 + s] = dN[r * 3 + s] * L.s_in[s];
            // with respect to the unit quaternion u = (w, x, y, z) ...
            float du[4];
            du[0] = 2.0f * (qz * (dR[3] - dR[1]) + qy * (dR[2] - dR[6]) + qx * (dR[7] - dR[5]));
            du[1] = 2.0f * (qy * (dR[1] + dR[3]) + qz * (dR[2] + dR[6]) + qw * (dR[7] - dR[5]) -
                            2.0f * qx * (dR[4] + dR[8]));
            du[2] = 2.0f * (qx * (dR[1] + dR[3]) + qz * (dR[5] + dR[7]) + qw * (dR[2] - dR[6]) -
                            2.0f * qy * (dR[0] + dR[8]));
            du[3] = 2.0f * (qx * (dR[2] + dR[6]) + qy * (dR[5] + dR[7]) + qw * (dR[3] - dR[1]) -
                            2.0f * qz * (dR[0] + dR[4]));
            // ... and through the normalisation u = q / |q|: dq = (du - u (u . du)) / |q|
            const float dot = qw * du[0] + qx * du[1] + qy * du[2] + qz * du[3];
            G.add(out.d_rot, 0, (du[0] - qw * dot) * iqn);
            G.add(out.d_rot, 1, (du[1] - qx * dot) * iqn);
            G.add(out.d_rot, 2, (du[2] - qy * dot) * iqn);
            G.add(out.d_rot, 3, (du[3] - qz * dot) * iqn);
        }
    }

    // ---- colour: c_ch = clamp(sum_k B_k(dir) sh[3 k + ch] + 0.5), dir = (p - campos) / |.| ----
    if (g_col[0] != 0.0f || g_col[1] != 0.0f || g_col[2] != 0.0f) {
        float dir[3] = {L.gx - fr.campos[0], L.gy - fr.campos[1], L.gz - fr.campos[2]};
        const float nn = sqrtf(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2]);
        if (nn > 1e-8f) {
            dir[0] /= nn; dir[1] /= nn; dir[2] /= nn;
        } else {
            dir[0] = 0.0f; dir[1] = 0.0f; dir[2] = 0.0f;
        }
        ShDir d;
        d.x = dir[0]; d.y = dir[1]; d.z = dir[2];
        d.xx = d.x * d.x; d.yy = d.y * d.y; d.zz = d.z * d.z;
        d.xy = d.x * d.y; d.yz = d.y * d.z; d.xz = d.x * d.z;
        // first sweep over the coefficients, streamed: the unclamped colours and, per channel,
        // sum_k dB_k sh[3 k + ch]
        float cc[3] = {0.0f, 0.0f, 0.0f}, dd[3][3] = {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};
#pragma unroll
        for (int k = 0; k < kCoef; k++) {
            float B, dB[3];
            sh_basis(k, d, B, dB);
#pragma unroll
            for (int ch = 0; ch < 3; ch++) {
                const float s = kEarlySH ? L.sh_in[3 * k + ch] : A(GSR_A_SH0 + 3 * k + ch);
                cc[ch] += B * s;
                dd[ch][0] += dB[0] * s; dd[ch][1] += dB[1] * s; dd[ch][2] += dB[2] * s;
            }
        }
        // the clamp passes gradient only strictly inside
        float gc[3];
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const float v = cc[ch] + 0.5f;
            gc[ch] = (v > 0.0f && (SH3 || v < 1.0f)) ? g_col[ch] : 0.0f;
        }
        if (out.d_sh) {
#pragma unroll
            for (int k = 0; k < kCoef; k++) {
                float B, dB[3];
                sh_basis(k, d, B, dB);
#pragma unroll
                for (int ch = 0; ch < 3; ch++) G.add(out.d_sh, 3 * k + ch, gc[ch] * B);
            }
        }
        if (nn > 1e-8f) {
            float dv[3];
#pragma unroll
            for (int j = 0; j < 3; j++) dv[j] = gc[0] * dd[0][j] + gc[1] * dd[1][j] + gc[2] * dd[2][j];
            const float dot = dir[0] * dv[0] + dir[1] * dv[1] + dir[2] * dv[2];
#pragma unroll
            for (int j = 0; j < 3; j++) d_pos[j] += (dv[j] - dir[j] * dot) / nn;
        }
    }

    // ---- opacity (times the temporal factor of a 4D block) and the position's own arrays ----
    if (out.d_position) {
#pragma unroll
        for (int j = 0; j < 3; j++) G.add(out.d_position, j, d_pos[j]);
    }
    if (out.d_opacity) G.add(out.d_opacity, 0, T4D ? g_op * L.tfac : g_op);
    if (T4D && out.d_temporal) {
        // dt = t - c, p = x + m0 dt + m3 dt^2 + m6 dt^3, tfac = exp(-(dt / s)^2)
        const float dt = tnow - A(GSR_A_TCENTER);
        const float dt2 = dt * dt, dt3 = dt2 * dt;
        const float ts = A(GSR_A_TSCALE);
        const float u = dt / ts;
        const float d_u = (g_op * L.op_in) * L.tfac * (-2.0f * u);
        float d_dt = d_u / ts;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const float m0 = A(GSR_A_MOTION0 + j), m3 = A(GSR_A_MOTION0 + 3 + j), m6 = A(GSR_A_MOTION0 + 6 + j);
            d_dt += d_pos[j] * ((m0 + 2.0f * m3 * dt) + 3.0f * m6 * dt2);
            G.add(out.d_temporal, 2 + j, d_pos[j] * dt);
            G.add(out.d_temporal, 5 + j, d_pos[j] * dt2);
            G.add(out.d_temporal, 8 + j, d_pos[j] * dt3);
        }
        G.add(out.d_temporal, 0, -d_dt);
        G.add(out.d_temporal, 1, -(d_u * u) / ts);
    }
}

}  // namespace

hipError_t launch_project_backward(const float* arrays, int64_t stride, int64_t n, const Frame& fr, bool four_d,
                                   bool sh3, float t, const gsr_record_grads& in, const gsr_scene_grads& out,
                                   hipStream_t s, const float* in_z) {
    if (n <= 0) return hipSuccess;
    const int grid = grid_for(n, 256);
    with_bool(in_z != nullptr, [&](auto dz) {
        constexpr bool DZ = decltype(dz)::value;
        if (four_d)
            k_project_backward<true, false, DZ><<<grid, 256, 0, s>>>(arrays, stride, n, fr, t, in, out, in_z);
        else if (sh3)
            k_project_backward<false, true, DZ><<<grid, 256, 0, s>>>(arrays, stride, n, fr, t, in, out, in_z);
        else
            k_project_backward<false, false, DZ><<<grid, 256, 0, s>>>(arrays, stride, n, fr, t, in, out, in_z);
    });
    return hipGetLastError();
}

}  // namespace gsr

// gsr_preprocess_device.h — device code of the preprocess's map from scene arrays to splat
// record that its backward pass restates decisions of: the scene-array access, the loads, the
// world-space covariance, the small matrix products and the cull tests.  Shared by
// gsr_kernels.hip (k_preprocess, k_preprocess_multi) and gsr_project.hip (k_project_backward),
// so that both take every decision on the same float32 values.  gsr_scene_densify.hip
// (k_densify_split) takes the quaternion's rotation from here, so a split child moves along
// the axes the preprocess draws.
//
// Every float expression restates render.cu / math.cu in the same operation order (the
// translation units are compiled with -ffp-contract=off), and the transcendental functions
// come from gsr_detmath.h: the results are bit-identical to the CPU oracle.
#pragma once

#include "gsr_device.h"

namespace gsr {

namespace {

__constant__ float kShC0 = 0.28209479177387814f;      // render.cu:369-377
__constant__ float kShC1 = 0.4886025119029199f;

// math.cu:120-129 (matMul3D_cuda): out = 0; out += A[ik]*B[kj], k ascending.
__device__ __forceinline__ void mm3(const float* A, const float* B, float* out) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float acc = 0.0f;
#pragma unroll
            for (int k = 0; k < 3; ++k) acc += A[i * 3 + k] * B[k * 3 + j];
            out[i * 3 + j] = acc;
        }
}

// math.cu:172-186 (geMatMul_cuda), A MxK, B KxN.
template <int M, int N, int K>
__device__ __forceinline__ void gemm(const float* A, const float* B, float* out) {
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j) {
            float acc = 0.0f;
#pragma unroll
            for (int k = 0; k < K; ++k) acc += A[i * K + k] * B[k * N + j];
            out[i * N + j] = acc;
        }
}

// (matVecMul4D_cuda, mv4: gsr_device.h; k_aux_depth shares it)

// Array k of the scene block for the workgroup's Gaussians: the base (arr + k stride + the
// workgroup's first index) is uniform, so it is formed by scalar instructions and the load
// takes it as an SGPR pair beside the lane's 32-bit byte offset (global_load ... saddr).
// Indexing arr[k * stride + i] with a 64-bit i made every load's address a per-lane
// 64-bit multiply-add (v_mad_u64_u32) — ~150 VALU per Gaussian for 38 arrays.
struct SoaWg {
    const float* base;   // arr + first index of the workgroup (uniform)
    int64_t stride;
    uint32_t off;        // lane byte offset: 4 * (i - first index)
    __device__ __forceinline__ float operator()(int64_t k) const {
        typedef const __attribute__((address_space(1))) char* gptr;
        gptr b = (gptr)(base + k * stride);
        asm("" : "+s"(b));   // keep the base whole (the compiler re-associates it into the lane part)
        return *(const __attribute__((address_space(1))) float*)(b + off);
    }
};

// preprocess_one in three parts, shared with k_preprocess_multi: the loads
// (preprocess_load), the view-independent arithmetic (preprocess_cov3d and the opacity-only
// terms, PreShared) and everything that depends on the camera (preprocess_camera).
template <bool T4D, bool SH3>
struct PreLoads {
    // Every load of the Gaussian but the late SH is issued before the cull decides
    // whether it is needed: one memory round trip instead of three (position, then
    // rotation / scale, then SH).  Wasted bytes for culled Gaussians only (config 2:
    // 5 %).  The SH stays behind the cull in 4D (the temporal cull drops ~64 %) and
    // SH-3 (48 coefficients) modes.
    static constexpr bool kEarlySH = !T4D && !SH3;
    float gx, gy, gz, tfac;
    float q_in[4], s_in[3], op_in, sh_in[kEarlySH ? 27 : 1];
};

// Temporal state of a 4D (Spacetime-Gaussian style) Gaussian at time t, in
// this exact operation order (the oracle restates it, oracle/gsr_oracle.c):
// dt = t - c; x_t = ((x + m0 dt) + m3 dt^2) + m6 dt^3 (dt^2 = dt dt, dt^3 =
// dt^2 dt; y, z with m1/m4/m7, m2/m5/m8); temporal factor exp(-(dt/s)^2).
template <bool T4D, bool SH3>
__device__ __forceinline__ void preprocess_load(const SoaWg& A, float tnow, PreLoads<T4D, SH3>& L) {
    float gx = A(GSR_A_X);
    float gy = A(GSR_A_Y);
    float gz = A(GSR_A_Z);
    float tfac = 1.0f;
    if (T4D) {
        const float dt = tnow - A(GSR_A_TCENTER);
        const float dt2 = dt * dt, dt3 = dt2 * dt;
        auto m = [&](int j) { return A(GSR_A_MOTION0 + j); };
        gx = ((gx + m(0) * dt) + m(3) * dt2) + m(6) * dt3;
        gy = ((gy + m(1) * dt) + m(4) * dt2) + m(7) * dt3;
        gz = ((gz + m(2) * dt) + m(5) * dt2) + m(8) * dt3;
        const float u = dt / A(GSR_A_TSCALE);
        tfac = gsr_expf(-(u * u));
    }
    L.gx = gx; L.gy = gy; L.gz = gz; L.tfac = tfac;
#pragma unroll
    for (int k = 0; k < 4; k++) L.q_in[k] = A(GSR_A_ROT0 + k);
#pragma unroll
    for (int k = 0; k < 3; k++) L.s_in[k] = A(GSR_A_SCALE0 + k);
    L.op_in = A(GSR_A_OPACITY);
    if (PreLoads<T4D, SH3>::kEarlySH) {
#pragma unroll
        for (int k = 0; k < 27; k++) L.sh_in[k] = A(GSR_A_SH0 + k);
    }
}

// Rotation matrix (row-major) of the normalised quaternion q_in = (w, x, y, z):
// buildRotMatFromQuat_cuda (math.cu:153-164).  Shared with the densification's split kernel
// (gsr_scene_densify.hip), which offsets a child along the same axes the preprocess draws.
__device__ __forceinline__ void quat_rotation(const float* q_in, float* Rm) {
    float qw = q_in[0];
    float qx = q_in[1];
    float qy = q_in[2];
    float qz = q_in[3];
    const float qn = sqrtf(qx * qx + qy * qy + qz * qz + qw * qw);
    qx /= qn; qy /= qn; qz /= qn; qw /= qn;
    Rm[0] = 1 - 2 * qy * qy - 2 * qz * qz; Rm[1] = 2 * qx * qy - 2 * qw * qz;     Rm[2] = 2 * qx * qz + 2 * qw * qy;
    Rm[3] = 2 * qx * qy + 2 * qw * qz;     Rm[4] = 1 - 2 * qx * qx - 2 * qz * qz; Rm[5] = 2 * qy * qz - 2 * qw * qx;
    Rm[6] = 2 * qx * qz - 2 * qw * qy;     Rm[7] = 2 * qy * qz + 2 * qw * qx;     Rm[8] = 1 - 2 * qx * qx - 2 * qy * qy;
}

// World-space covariance R S S R^T of one Gaussian (render.cu:655-686, the part before
// the camera rotation).
__device__ __forceinline__ void preprocess_cov3d(const float* q_in, const float* s_in, float* cov) {
    float Rm[9], RT[9], S[9], tmp[9];
    quat_rotation(q_in, Rm);
    RT[0] = Rm[0]; RT[1] = Rm[3]; RT[2] = Rm[6];
    RT[3] = Rm[1]; RT[4] = Rm[4]; RT[5] = Rm[7];
    RT[6] = Rm[2]; RT[7] = Rm[5]; RT[8] = Rm[8];
    S[0] = s_in[0]; S[1] = 0.0f; S[2] = 0.0f;
    S[3] = 0.0f; S[4] = s_in[1]; S[5] = 0.0f;
    S[6] = 0.0f; S[7] = 0.0f; S[8] = s_in[2];
    mm3(Rm, S, tmp);
    mm3(tmp, S, Rm);
    mm3(Rm, RT, cov);
}

// The tests after which no splat record exists (status 0 of the oracle), on the preprocess's
// own float32 values: a non-finite view position (render.cu:543); non-finite ndc, a Gaussian
// not in front of the near plane, ndc z outside [-1, 1] (render.cu:553-556); a 2D covariance
// (in pixels) with a non-finite or too small determinant (render.cu:690).  Macros, not
// functions: as bool-returning inline functions they changed k_preprocess's instructions
// (tools/kernel_isa_diff.py), as the same expression in place they do not.
#define GSR_VIEW_CULLED(view) (!isfinite((view)[0]) || !isfinite((view)[1]) || !isfinite((view)[2]))
#define GSR_CLIP_CULLED(fr, view, ndc)                                             \
    (!isfinite((ndc)[0]) || !isfinite((ndc)[1]) || !isfinite((ndc)[2]) ||          \
     (view)[2] >= -(fr).znear || (ndc)[2] < -1.0f || (ndc)[2] > 1.0f)
#define GSR_DET_CULLED(det) (!isfinite(det) || (det) < 1e-8f)

}  // namespace

}  // namespace gsr

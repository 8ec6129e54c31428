// gsr_camera.cpp — the camera helpers of include/gsr.h, which mirror the reference's camera.cpp
// and math.cpp.  Host arithmetic only: no context, no device.
#include <cmath>
#include <cstring>

#include "gsr.h"

namespace {

void m_normalize(float v[3]) {   // math.cpp:7-20
    float nrm = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (nrm > 1e-8f) {
        v[0] /= nrm;
        v[1] /= nrm;
        v[2] /= nrm;
    } else {
        v[0] = 0.0f;
        v[1] = 0.0f;
        v[2] = 0.0f;
    }
}
float m_norm(const float v[3]) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }
void m_cross(const float a[3], const float b[3], float o[3]) {   // math.cpp:45-49
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
void m_sub(const float a[3], const float b[3], float o[3]) {
    o[0] = a[0] - b[0];
    o[1] = a[1] - b[1];
    o[2] = a[2] - b[2];
}
void m_view(const float x[3], const float y[3], const float z[3], const float e[3], float o[16]) {  // math.cpp:65-90
    o[0] = x[0]; o[1] = x[1]; o[2] = x[2]; o[3] = -(x[0] * e[0] + x[1] * e[1] + x[2] * e[2]);
    o[4] = y[0]; o[5] = y[1]; o[6] = y[2]; o[7] = -(y[0] * e[0] + y[1] * e[1] + y[2] * e[2]);
    o[8] = z[0]; o[9] = z[1]; o[10] = z[2]; o[11] = -(z[0] * e[0] + z[1] * e[1] + z[2] * e[2]);
    o[12] = 0.0f; o[13] = 0.0f; o[14] = 0.0f; o[15] = 1.0f;
}
void m_persp(float fovY, float aspect, float nr, float fr, float o[16]) {   // math.cpp:91-97
    float f = 1.0f / std::tan(fovY * 0.5f * (M_PI / 180.0f));
    o[0] = f / aspect; o[1] = 0.0f; o[2] = 0.0f; o[3] = 0.0f;
    o[4] = 0.0f; o[5] = f; o[6] = 0.0f; o[7] = 0.0f;
    o[8] = 0.0f; o[9] = 0.0f; o[10] = (fr + nr) / (nr - fr); o[11] = (2 * fr * nr) / (nr - fr);
    o[12] = 0.0f; o[13] = 0.0f; o[14] = -1.0f; o[15] = 0.0f;
}
void m_mm4(const float A[16], const float B[16], float o[16]) {   // math.cpp:99-108
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            o[i * 4 + j] = 0.0f;
            for (int k = 0; k < 4; ++k) o[i * 4 + j] += A[i * 4 + k] * B[k * 4 + j];
        }
}

}  // namespace

extern "C" void gsr_camera_default(gsr_camera* c) {   // camera.cpp:8-13
    std::memset(c, 0, sizeof *c);
    c->fovY = 45.0f;
    c->aspectRatio = 1.0f;
    c->nearClip = 0.1f;
    c->farClip = 100.0f;
    c->position[2] = 5.0f;
    c->up_vec[1] = 1.0f;
    c->w_up[1] = 1.0f;
}

extern "C" void gsr_camera_update(gsr_camera* c) {   // camera.cpp:36-57
    m_sub(c->lookAt, c->position, c->f_axis);
    m_normalize(c->f_axis);
    m_cross(c->f_axis, c->w_up, c->r_axis);
    m_normalize(c->r_axis);
    m_cross(c->r_axis, c->f_axis, c->u_axis);
    for (int i = 0; i < 3; i++) c->f_axis[i] = -c->f_axis[i];
    for (int i = 0; i < 3; i++) {
        c->r_cam[i] = c->r_axis[i];
        c->r_cam[3 + i] = c->u_axis[i];
        c->r_cam[6 + i] = c->f_axis[i];
    }
    const float* A = c->r_cam;
    float* T = c->r_cam_T;
    T[0] = A[0]; T[1] = A[3]; T[2] = A[6];
    T[3] = A[1]; T[4] = A[4]; T[5] = A[7];
    T[6] = A[2]; T[7] = A[5]; T[8] = A[8];
    m_view(c->r_axis, c->u_axis, c->f_axis, c->position, c->V_matrix);
    m_persp(c->fovY, c->aspectRatio, c->nearClip, c->farClip, c->P_matrix);
    m_mm4(c->P_matrix, c->V_matrix, c->M_matrix);
}

extern "C" void gsr_camera_update_frustum(gsr_camera* c) {   // camera.cpp:59-121
    float* pl = c->plane_normals;
    const float* f = c->f_axis;
    const float* p = c->position;
    for (int i = 0; i < 3; i++) pl[i] = f[i];
    pl[3] = (f[0] * p[0] + f[1] * p[1] + f[2] * p[2] - c->nearClip);
    for (int i = 0; i < 3; i++) pl[4 + i] = -f[i];
    pl[7] = -(f[0] * p[0] + f[1] * p[1] + f[2] * p[2] - c->farClip);
    float t_y = std::tan(c->fovY * 0.5f * (M_PI / 180.0f));
    float t_x = t_y * c->aspectRatio;
    const float sgn[4] = {-1.0f, 1.0f, -1.0f, 1.0f};
    for (int q = 0; q < 4; q++) {
        const float* ax = (q < 2) ? c->r_axis : c->u_axis;
        const float tt = (q < 2) ? t_x : t_y;
        float nrm[3];
        for (int i = 0; i < 3; i++) nrm[i] = (sgn[q] < 0) ? (f[i] * tt - ax[i]) : (f[i] * tt + ax[i]);
        m_normalize(nrm);
        for (int i = 0; i < 3; i++) pl[8 + 4 * q + i] = nrm[i];
        pl[11 + 4 * q] = 0.0f;
    }
}

extern "C" void gsr_camera_zoom(gsr_camera* c, float delta) {   // camera.cpp:123-128
    for (int i = 0; i < 3; i++) c->position[i] += c->f_axis[i] * delta;
    gsr_camera_update(c);
}

extern "C" void gsr_camera_orbit(gsr_camera* c, float azimuth, float elevation) {   // camera.cpp:130-158
    azimuth = azimuth * M_PI / 180.0f;
    elevation = elevation * M_PI / 180.0f;
    float rv[3];
    m_sub(c->position, c->lookAt, rv);
    float radius = m_norm(rv);
    float theta = std::atan2(rv[2], rv[0]);
    float phi = std::acos(rv[1] / radius);
    theta += azimuth;
    phi += elevation;
    const float epsilon = 0.01f;
    if (phi < epsilon) phi = epsilon;
    if (phi > M_PI - epsilon) phi = M_PI - epsilon;
    rv[0] = radius * std::sin(phi) * std::cos(theta);
    rv[1] = radius * std::cos(phi);
    rv[2] = radius * std::sin(phi) * std::sin(theta);
    for (int i = 0; i < 3; i++) c->position[i] = c->lookAt[i] + rv[i];
    gsr_camera_update(c);
}

extern "C" void gsr_camera_intrinsics(const gsr_camera* cam, float* fx, float* fy) {
    // render.cu:620-621: fy = 1/tanf(fovY*0.5f*(CUDART_PI_F/180.0f)); tanf taken
    // correctly rounded (float(tan(double))) so the oracle computes the same.
    const float PI_F = 3.141592654f;
    const float arg = cam->fovY * 0.5f * (PI_F / 180.0f);
    const float t = (float)std::tan((double)arg);
    *fy = 1.0f / t;
    *fx = *fy / cam->aspectRatio;
}

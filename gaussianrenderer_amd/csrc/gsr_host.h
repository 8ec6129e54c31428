// gsr_host.h — what the host translation units behind include/gsr.h share (gsr_runtime.cpp, the
// frame pipeline; gsr_scene.cpp, the context-free scene API; gsr_scene_save.cpp, the scene export): the error macros, the owned device
// allocation and a scene block's two facts of shape.  Host only: the host/kernel boundary is
// gsr_internal.h.  The thread's message itself (gsr::set_error, gsr_last_error) lives in
// gsr_runtime.cpp.
#pragma once

#include <cstddef>
#include <cstdint>
#include <utility>

#include <hip/hip_runtime.h>

#include "gsr.h"
#include "gsr_internal.h"

#define set_err gsr::set_error

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return set_err(GSR_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                           __FILE__, __LINE__);                                              \
    } while (0)

namespace {   // internal linkage: the instantiations stay out of libgsr.so's exported symbols

// One owned device allocation, freed with its owner.  Converts to T* so launch sites pass it
// like the raw pointer; move-only, swappable (switch_pre_set swaps the preprocess sets).
template <typename T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        std::swap(p_, o.p_);
        return *this;
    }
    ~DevBuf() {
        if (p_) (void)hipFree(p_);
    }
    operator T*() const { return p_; }
    T* get() const { return p_; }
    // Frees what it held, then allocates count elements (0: one); null when hipMalloc fails.
    int alloc(size_t count) {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        if (count == 0) count = 1;
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&p_), sizeof(T) * count));
        return GSR_OK;
    }

private:
    T* p_ = nullptr;
};

}  // namespace

// A scene block (gsr_scene_header, then narrays arrays): the arrays' stride in floats for n
// Gaussians, and where the arrays start.
inline int64_t scene_stride(int64_t n) { return (n + 63) / 64 * 64; }
inline float* scene_arrays(void* d) { return reinterpret_cast<float*>(static_cast<char*>(d) + GSR_SCENE_HEADER_BYTES); }
inline const float* scene_arrays(const void* d) {
    return reinterpret_cast<const float*>(static_cast<const char*>(d) + GSR_SCENE_HEADER_BYTES);
}

// A device scene block's header against (narrays, n) and its magic; GSR_OK, or GSR_E_ARG /
// GSR_E_HIP with the message set, `who` naming the call (gsr_scene.cpp).
int check_scene_block(const void* d_scene, int narrays, int64_t n, const char* who);

// gsr_host.h — what the host translation units behind include/gsr.h share (gsr_runtime.cpp, the
// frame pipeline; gsr_path.cpp, the frames in flight; gsr_inspect.cpp, readback, timing, tuning
// and the device probes; gsr_compat.cpp, the reference's own entry points; gsr_scene.cpp, the
// context-free scene API; gsr_scene_save.cpp, the scene export): the error macros, the owned
// device allocation and a scene block's two facts of shape.  Host only: the host/kernel boundary
// is gsr_internal.h; the context itself is gsr_context.h.  The thread's message (gsr::set_error,
// gsr_last_error) lives in gsr_runtime.cpp.
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

namespace gsr {

// One owned device allocation, freed with its owner, that knows how many elements it was last
// asked for.  Converts to T* so launch sites pass it like the raw pointer; move-only, swappable
// (switch_pre_set swaps the preprocess sets).  A member of gsr_context, which several
// translation units define, so it has a name with linkage; hidden visibility keeps its
// instantiations out of libgsr.so's exported symbols.
template <typename T>
class __attribute__((visibility("hidden"))) DevBuf {
public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) {
        o.p_ = nullptr;
        o.cap_ = 0;
    }
    DevBuf& operator=(DevBuf&& o) noexcept {
        std::swap(p_, o.p_);
        std::swap(cap_, o.cap_);
        return *this;
    }
    ~DevBuf() {
        if (p_) (void)hipFree(p_);
    }
    operator T*() const { return p_; }
    T* get() const { return p_; }
    // Elements the last alloc was asked for: 0 when empty, and 0 after an alloc that failed.
    size_t capacity() const { return cap_; }
    // Frees what it held, then allocates count elements (0: one); null when hipMalloc fails.
    int alloc(size_t count) {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        cap_ = 0;
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&p_), sizeof(T) * (count ? count : 1)));
        cap_ = count;
        return GSR_OK;
    }
    // Grows to count elements (the old content is lost); the device is drained first, since
    // work queued on any stream may still use the old allocation.
    int reserve(size_t count) {
        if (count <= cap_) return GSR_OK;
        HIP_TRY(hipDeviceSynchronize());
        return alloc(count);
    }

private:
    T* p_ = nullptr;
    size_t cap_ = 0;
};

// Workgroups for n items at `per` items each, 1..kMaxSortGroups.
inline int groups_for(int64_t n, int64_t per) {
    const int64_t g = (n + per - 1) / per;
    return (int)(g < 1 ? 1 : g > kMaxSortGroups ? kMaxSortGroups : g);
}

}  // namespace gsr

using gsr::DevBuf;

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

// gsr_compat.cpp — the reference's own entry points: the viewer's drop-in frame call
// (preprocessCUDAGaussians; its GL form is gsr_gl.cpp) and the two host-array sort calls.  Built
// on the public API of include/gsr.h and the kernel launchers; it never looks inside a context.
#include <algorithm>
#include <cstdio>
#include <mutex>
#include <utility>

#include "gsr_host.h"

// ------------------------------------------------------------------ drop-in render

static std::mutex g_dropin_mu;

// The drop-in calls' context and the host-image call's device image, created at the first call
// and never destroyed: a static object's destructor would call hipFree while the process exits,
// when the HIP runtime may already be gone.
struct DropIn {
    gsr_context* ctx;
    DevBuf<float> out;
};
static DropIn* g_dropin = nullptr;
static DropIn& dropin() {
    if (!g_dropin) g_dropin = new DropIn{gsr_create(), {}};
    return *g_dropin;
}

// Whole drop-in frame into a DEVICE image (3*W*H floats) on the drop-in
// context, synchronous like the reference call: scene-layout detection from the
// block header, and up to two re-renders after a pair-buffer overflow.  Shared by
// preprocessCUDAGaussians (host image) and preprocessCUDAGaussiansGL (the
// viewer's SSBO, gsr_gl.cpp).  Returns a GSR_* code; `what` names the failing step.
int gsr::dropin_render_device(gsr_gaussian* d_gaussians, int num_gaussians, const gsr_camera& cam,
                              int num_tile_y, int num_tile_x, int width_stride, int height_stride, int W,
                              int H, float k, float* d_out, const char** what) {
    *what = "render";
    gsr_context* c = dropin().ctx;
    // Layout detection: our scene block starts with a NaN-pattern magic.
    int layout = GSR_LAYOUT_AOS;
    if (num_gaussians > 0 && d_gaussians) {
        gsr_scene_header h{};
        *what = "scene";
        // One synchronous read (~16 us each on the viewer's frame): the whole header
        // when even an AoS buffer of num_gaussians records is at least that long (2+
        // records), else the magic first (16 B fit inside any 240-B AoS record) and the
        // rest of the header only once it is known to be our block.
        const bool whole = (int64_t)num_gaussians * (int64_t)sizeof(gsr_gaussian) >= (int64_t)sizeof h;
        HIP_TRY(hipMemcpy(whole ? static_cast<void*>(&h) : static_cast<void*>(&h.magic), d_gaussians,
                          whole ? sizeof h : sizeof h.magic, hipMemcpyDeviceToHost));
        if (h.magic[0] == GSR_SCENE_MAGIC0 && h.magic[1] == GSR_SCENE_MAGIC1 && h.magic[2] == GSR_SCENE_MAGIC2 &&
            h.magic[3] == GSR_SCENE_MAGIC3) {
            if (!whole) HIP_TRY(hipMemcpy(&h, d_gaussians, sizeof h, hipMemcpyDeviceToHost));
            // 4D blocks render at the drop-in context's time (gsr_set_time on it is not
            // reachable through this ABI, so t = 0: the sequence's first frame)
            layout = h.narrays == GSR_SCENE4D_NARRAYS    ? GSR_LAYOUT_SCENE_BLOCK_4D
                     : h.narrays == GSR_SCENE_SH3_NARRAYS ? GSR_LAYOUT_SCENE_BLOCK_SH3
                                                         : GSR_LAYOUT_SCENE_BLOCK;
            if ((int64_t)h.count != num_gaussians)
                return set_err(GSR_E_ARG, "num_gaussians %d != scene block count %llu", num_gaussians,
                               (unsigned long long)h.count);
        }
    }
    for (int attempt = 0; attempt < 3; attempt++) {
        *what = "render";
        int rc = gsr_render(c, d_gaussians, layout, num_gaussians, &cam, W, H, num_tile_x, num_tile_y,
                            width_stride, height_stride, k, d_out, nullptr);
        if (rc != GSR_OK && rc != GSR_E_OVERFLOW) return rc;
        *what = "sync";
        rc = gsr_sync(c);
        if (rc != GSR_E_OVERFLOW) return rc;
    }
    // each overflow grows the buffer to 1.25x the frame's pair count, so a repeat
    // means the scene or camera changed under us: report it, never a partial image
    return set_err(GSR_E_OVERFLOW, "pair buffer still overflowing after 3 renders");
}

extern "C" void preprocessCUDAGaussians(gsr_gaussian* d_gaussians, float* out_pixels, int num_gaussians,
                                        gsr_camera cam, int num_tile_y, int num_tile_x, int width_stride,
                                        int height_stride, int tile_W, int tile_H, float k) {
    std::lock_guard<std::mutex> lk(gsr::dropin_mutex());
    auto fail = [](const char* what) { std::fprintf(stderr, "preprocessCUDAGaussians: %s: %s\n", what, gsr::last_error()); };
    if (!out_pixels || tile_W <= 0 || tile_H <= 0) {
        set_err(GSR_E_ARG, "bad output buffer or size");
        fail("argument");
        return;
    }
    DevBuf<float>& out = dropin().out;
    const size_t npx = 3 * (size_t)tile_W * (size_t)tile_H;
    if (out.capacity() < npx) {
        if (out.alloc(npx)) { fail("alloc"); return; }
    }
    const char* what = "render";
    if (gsr::dropin_render_device(d_gaussians, num_gaussians, cam, num_tile_y, num_tile_x, width_stride,
                                  height_stride, tile_W, tile_H, k, out, &what) != GSR_OK) {
        fail(what);
        return;
    }
    if (hipMemcpy(out_pixels, out, npx * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) {
        set_err(GSR_E_HIP, "image readback failed");
        fail("readback");
    }
}

std::mutex& gsr::dropin_mutex() { return g_dropin_mu; }

// ------------------------------------------------------------------ reference sort ABI
//
// Both entry points take HOST arrays like the reference (they copy H2D, sort,
// copy D2H) and report the device time of the sort passes in *kernel_ms
// (cudaEvent bracket of render.cu:221-253 / onesweep.cu:217-240).

namespace {

struct SortBufs {
    DevBuf<uint64_t> a, b, c;
    DevBuf<uint32_t> hist, totals;
    int alloc(uint32_t n, bool third) {
        if (int rc = a.alloc(n)) return rc;
        if (int rc = b.alloc(n)) return rc;
        if (third) {
            if (int rc = c.alloc(n)) return rc;
        }
        if (int rc = hist.alloc(256 * (size_t)gsr::kMaxSortGroups)) return rc;
        return totals.alloc(256);
    }
};

// Stable sort of n items on bits [32, 32 + nbits); returns the buffer holding the result.
int sort_high_bits(SortBufs& sb, uint64_t* a, uint64_t* b, uint32_t n, int nbits, uint64_t** result) {
    const int g = gsr::groups_for(n, gsr::kSortTile);
    uint64_t* src = a;
    uint64_t* dst = b;
    for (int sh = 0; sh < nbits; sh += 8) {
        HIP_TRY(gsr::launch_radix_pass(src, dst, nullptr, n, 32 + sh, std::min(8, nbits - sh), g, 16, sb.hist,
                                       sb.totals, nullptr, nullptr));
        std::swap(src, dst);
    }
    *result = src;
    return GSR_OK;
}

// The one way out of a sort entry point, whatever `rc` its body returned: the two timing
// events go, and an error is printed.
void sort_done(const char* who, int rc, hipEvent_t e0, hipEvent_t e1) {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (rc != GSR_OK) std::fprintf(stderr, "%s: %s\n", who, gsr::last_error());
}

}  // namespace

extern "C" void oneSweepSort(int* input, int* output, int N, int maxVal, float* kernel_ms) {
    (void)maxVal;   // the reference sorts all 32 bits regardless (onesweep.cu:197-198)
    if (kernel_ms) *kernel_ms = 0.0f;
    if (N <= 0) return;
    if (!input || !output) {
        std::fprintf(stderr, "oneSweepSort: null buffer\n");
        return;
    }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto body = [&]() -> int {
        SortBufs sb;
        if (int rc = sb.alloc((uint32_t)N, false)) return rc;
        DevBuf<int> dkeys;
        if (int rc = dkeys.alloc((size_t)N)) return rc;
        HIP_TRY(hipMemcpy(dkeys, input, sizeof(int) * (size_t)N, hipMemcpyHostToDevice));
        HIP_TRY(hipEventCreate(&e0));
        HIP_TRY(hipEventCreate(&e1));
        HIP_TRY(hipEventRecord(e0, nullptr));
        HIP_TRY(gsr::launch_items_from_keys(dkeys, (uint32_t)N, sb.a, nullptr));
        uint64_t* res = nullptr;
        if (int rc = sort_high_bits(sb, sb.a, sb.b, (uint32_t)N, 32, &res)) return rc;
        HIP_TRY(gsr::launch_keys_from_items(res, (uint32_t)N, dkeys, nullptr));
        HIP_TRY(hipEventRecord(e1, nullptr));
        HIP_TRY(hipEventSynchronize(e1));
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        if (kernel_ms) *kernel_ms = ms;
        HIP_TRY(hipMemcpy(output, dkeys, sizeof(int) * (size_t)N, hipMemcpyDeviceToHost));
        return GSR_OK;
    };
    const int rc = body();   // before e0 and e1 are read
    sort_done("oneSweepSort", rc, e0, e1);
}

extern "C" void oneSweep3DGaussianSort(gsr_lwg* d_in, int N, int num_bits, float* kernel_ms) {
    if (kernel_ms) *kernel_ms = 0.0f;
    if (N <= 0) return;
    if (!d_in || num_bits <= 0 || num_bits > 64) {
        std::fprintf(stderr, "oneSweep3DGaussianSort: bad argument\n");
        return;
    }
    // numPasses = (num_bits + 7) / 8 full 8-bit digits (render.cu:201): sort on
    // the low 8*numPasses bits of radix_id, stable, values travel with keys.
    const int nb = 8 * ((num_bits + 7) / 8);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto body = [&]() -> int {
        SortBufs sb;
        if (int rc = sb.alloc((uint32_t)N, true)) return rc;
        DevBuf<gsr_lwg> din, dout;
        if (int rc = din.alloc((size_t)N)) return rc;
        if (int rc = dout.alloc((size_t)N)) return rc;
        HIP_TRY(hipMemcpy(din, d_in, sizeof(gsr_lwg) * (size_t)N, hipMemcpyHostToDevice));
        HIP_TRY(hipEventCreate(&e0));
        HIP_TRY(hipEventCreate(&e1));
        HIP_TRY(hipEventRecord(e0, nullptr));
        // stage 1: low min(32, nb) bits
        const int b1 = std::min(32, nb);
        HIP_TRY(gsr::launch_items_from_lwg(din, nullptr, (uint32_t)N, 0, b1 == 32 ? 0xffffffffu : ((1u << b1) - 1u),
                                           sb.a, nullptr));
        uint64_t* r1 = nullptr;
        if (int rc = sort_high_bits(sb, sb.a, sb.b, (uint32_t)N, b1, &r1)) return rc;
        const uint64_t* s1 = nullptr;
        const uint64_t* s2 = r1;
        if (nb > 32) {
            // stage 2: bits [32, nb), stable over the stage-1 order (LSD composition)
            const int b2 = nb - 32;
            uint64_t* spare = (r1 == sb.a) ? sb.b : sb.a;
            HIP_TRY(gsr::launch_items_from_lwg(din, r1, (uint32_t)N, 32, b2 == 32 ? 0xffffffffu : ((1u << b2) - 1u),
                                               sb.c, nullptr));
            uint64_t* r2 = nullptr;
            if (int rc = sort_high_bits(sb, sb.c, spare, (uint32_t)N, b2, &r2)) return rc;
            s1 = r1;
            s2 = r2;
        }
        HIP_TRY(gsr::launch_gather_lwg(din, s1, s2, (uint32_t)N, dout, nullptr));
        HIP_TRY(hipEventRecord(e1, nullptr));
        HIP_TRY(hipEventSynchronize(e1));
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        if (kernel_ms) *kernel_ms = ms;
        HIP_TRY(hipMemcpy(d_in, dout, sizeof(gsr_lwg) * (size_t)N, hipMemcpyDeviceToHost));
        return GSR_OK;
    };
    const int rc = body();   // before e0 and e1 are read
    sort_done("oneSweep3DGaussianSort", rc, e0, e1);
}

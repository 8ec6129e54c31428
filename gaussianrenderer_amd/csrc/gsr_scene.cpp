// gsr_scene.cpp — the context-free scene API of include/gsr.h: device scene blocks (upload, copy,
// download), scene editing, the Adam step, densification, initialisation from a point cloud, the
// image loss and the PLY-to-device loaders (gsr_load_ply_device, loadGaussianCudaFromPly).  None
// of it needs a gsr_context: every call checks its arguments before any device work, then is
// ordered on the caller's stream.  The argument checks share one definition per idiom (below);
// every message is pinned byte for byte by tests/test_scene_api_errors.py.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "gsr_host.h"
#include "gsr_detmath.h"

// ------------------------------------------------------------------ shared checks

namespace {

// The failure exit of an entry point that returns a block: `return null_err(set_err(...));`,
// or null_err(rc) after a callee that has set the message.
void* null_err(int) { return nullptr; }

bool is_block_narrays(int narrays) {
    return narrays == GSR_SCENE_NARRAYS || narrays == GSR_SCENE4D_NARRAYS || narrays == GSR_SCENE_SH3_NARRAYS;
}
bool is_block_layout(int layout) {
    return layout == GSR_LAYOUT_SCENE_BLOCK || layout == GSR_LAYOUT_SCENE_BLOCK_4D || layout == GSR_LAYOUT_SCENE_BLOCK_SH3;
}
// A count the kernels index with 32 bits.
bool count_in_range(int64_t n) { return n >= 0 && n <= INT32_MAX; }

// Is any of the pointers (null ones aside) off a 4-byte boundary.
template <typename... Ts>
bool misaligned(const Ts*... p) {
    return ((reinterpret_cast<uintptr_t>(p) | ...) % 4) != 0;
}

// A new scene block, freed with its owner unless release() has handed it to the caller: no
// path between alloc() and a return leaks it.
class NewBlock {
public:
    NewBlock() = default;
    NewBlock(const NewBlock&) = delete;
    NewBlock& operator=(const NewBlock&) = delete;
    ~NewBlock() {
        if (d_) (void)hipFree(d_);
    }
    // gsr_scene_bytes(narrays, n) bytes (both checked by the caller); GSR_E_HIP with the message set.
    int alloc(int narrays, int64_t n) {
        const int64_t bytes = gsr_scene_bytes(narrays, n);
        hipError_t e = hipMalloc(&d_, (size_t)bytes);
        if (e == hipSuccess) return GSR_OK;
        d_ = nullptr;
        return set_err(GSR_E_HIP, "hipMalloc(%lld) failed: %s", (long long)bytes, hipGetErrorString(e));
    }
    void* get() const { return d_; }
    float* arrays() const { return scene_arrays(d_); }
    void* release() { return std::exchange(d_, nullptr); }

private:
    void* d_ = nullptr;
};

}  // namespace

// ------------------------------------------------------------------ device scene blocks

extern "C" void* gsr_scene_upload_ex(const float* host_soa, int narrays, int64_t n) {
    if (!count_in_range(n) || (n > 0 && !host_soa) || !is_block_narrays(narrays))
        return null_err(set_err(GSR_E_ARG, "gsr_scene_upload: bad argument"));
    const int64_t stride = scene_stride(n);
    NewBlock blk;
    if (int rc = blk.alloc(narrays, n)) return null_err(rc);
    gsr_scene_header h{};
    h.magic[0] = GSR_SCENE_MAGIC0;
    h.magic[1] = GSR_SCENE_MAGIC1;
    h.magic[2] = GSR_SCENE_MAGIC2;
    h.magic[3] = GSR_SCENE_MAGIC3;
    h.count = (uint64_t)n;
    h.stride = (uint64_t)stride;
    h.narrays = (uint64_t)narrays;
    hipError_t e = hipMemcpy(blk.get(), &h, sizeof h, hipMemcpyHostToDevice);
    if (e == hipSuccess && n > 0)
        e = hipMemcpy2D(blk.arrays(), sizeof(float) * (size_t)stride, host_soa, sizeof(float) * (size_t)n,
                        sizeof(float) * (size_t)n, (size_t)narrays, hipMemcpyHostToDevice);
    if (e != hipSuccess) return null_err(set_err(GSR_E_HIP, "scene upload failed: %s", hipGetErrorString(e)));
    return blk.release();
}

extern "C" int64_t gsr_scene_bytes(int narrays, int64_t n) {
    if (!count_in_range(n) || !is_block_narrays(narrays)) return set_err(GSR_E_ARG, "gsr_scene_bytes: bad argument");
    return (int64_t)GSR_SCENE_HEADER_BYTES + (int64_t)sizeof(float) * narrays * scene_stride(n);
}

extern "C" int gsr_scene_copy(void* d_dst, const void* d_scene, int narrays, int64_t n, void* stream) {
    const int64_t bytes = gsr_scene_bytes(narrays, n);
    if (bytes < 0) return (int)bytes;
    if (!d_dst || !d_scene) return set_err(GSR_E_ARG, "gsr_scene_copy: null pointer");
    gsr_scene_header h{};
    HIP_TRY(hipMemcpy(&h, d_scene, sizeof h, hipMemcpyDeviceToHost));
    if (h.count != (uint64_t)n || h.narrays != (uint64_t)narrays)
        return set_err(GSR_E_ARG, "gsr_scene_copy: block holds %llu Gaussians x %llu arrays, not %lld x %d",
                       (unsigned long long)h.count, (unsigned long long)h.narrays, (long long)n, narrays);
    HIP_TRY(hipMemcpyAsync(d_dst, d_scene, (size_t)bytes, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
    return GSR_OK;
}

// ---- scene editing (kernels: gsr_scene_ops.hip) ----

extern "C" int gsr_mask_indices(const uint8_t* d_keep, int64_t n, int32_t* d_indices, int64_t* m_out, void* stream) {
    if (!m_out) return set_err(GSR_E_ARG, "gsr_mask_indices: null m_out");
    if (!count_in_range(n)) return set_err(GSR_E_ARG, "gsr_mask_indices: n = %lld out of range", (long long)n);
    if (n == 0) {
        *m_out = 0;
        return GSR_OK;
    }
    if (!d_keep || !d_indices) return set_err(GSR_E_ARG, "gsr_mask_indices: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint32_t chunks = gsr::mask_chunks((uint32_t)n);
    DevBuf<uint32_t> counts;   // the chunk counts, then the total
    if (int rc = counts.alloc((size_t)chunks + 1)) return rc;
    uint32_t m = 0;
    hipError_t e = gsr::launch_mask_indices(d_keep, (uint32_t)n, counts, d_indices, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&m, counts + chunks, sizeof m, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return set_err(GSR_E_HIP, "gsr_mask_indices failed: %s", hipGetErrorString(e));
    *m_out = (int64_t)m;
    return GSR_OK;
}

extern "C" int gsr_gather_planes(void* d_dst, int64_t dst_stride, const void* d_src, int64_t src_stride, int nplanes,
                                 int elem_bytes, int64_t n, const int32_t* d_indices, int64_t m, uint32_t* d_bad,
                                 void* stream) {
    if (!d_dst || !d_src || !d_indices) return set_err(GSR_E_ARG, "gsr_gather_planes: null pointer");
    if (elem_bytes != 4 && elem_bytes != 8)
        return set_err(GSR_E_ARG, "gsr_gather_planes: elem_bytes = %d, not 4 or 8", elem_bytes);
    if (nplanes < 1) return set_err(GSR_E_ARG, "gsr_gather_planes: nplanes = %d < 1", nplanes);
    if (!count_in_range(n) || !count_in_range(m) || (m > 0 && n == 0))
        return set_err(GSR_E_ARG, "gsr_gather_planes: n = %lld, m = %lld out of range", (long long)n, (long long)m);
    if (src_stride < n || dst_stride < m)
        return set_err(GSR_E_ARG, "gsr_gather_planes: stride smaller than its count (src %lld < %lld or dst %lld < %lld)",
                       (long long)src_stride, (long long)n, (long long)dst_stride, (long long)m);
    if (((uintptr_t)d_dst | (uintptr_t)d_src) % (uintptr_t)elem_bytes || misaligned(d_indices, d_bad))
        return set_err(GSR_E_ARG, "gsr_gather_planes: misaligned pointer");
    HIP_TRY(gsr::launch_gather_planes(d_dst, dst_stride, d_src, src_stride, nplanes, elem_bytes, (uint32_t)n,
                                      d_indices, (uint32_t)m, d_bad, nullptr, static_cast<hipStream_t>(stream)));
    return GSR_OK;
}

// The source block's header against (narrays, n), as gsr_scene_copy checks it, and its magic
// (an AoS array is refused).  Synchronous 256-byte read.  (Declared in gsr_host.h: gsr_scene_save.cpp
// checks its source with it too.)
int check_scene_block(const void* d_scene, int narrays, int64_t n, const char* who) {
    gsr_scene_header h{};
    hipError_t e = hipMemcpy(&h, d_scene, sizeof h, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return set_err(GSR_E_HIP, "%s: reading the header failed: %s", who, hipGetErrorString(e));
    if (h.magic[0] != GSR_SCENE_MAGIC0 || h.magic[1] != GSR_SCENE_MAGIC1 || h.magic[2] != GSR_SCENE_MAGIC2 ||
        h.magic[3] != GSR_SCENE_MAGIC3)
        return set_err(GSR_E_ARG, "%s: not a scene block (an AoS array?)", who);
    if (h.count != (uint64_t)n || h.narrays != (uint64_t)narrays || h.stride != (uint64_t)scene_stride(n))
        return set_err(GSR_E_ARG, "%s: block holds %llu Gaussians x %llu arrays, not %lld x %d", who,
                       (unsigned long long)h.count, (unsigned long long)h.narrays, (long long)n, narrays);
    return GSR_OK;
}

// gsr_scene_gather after its argument and header checks.
static void* scene_gather_checked(const void* d_scene, int narrays, int64_t n, const int32_t* d_indices, int64_t m,
                                  uint32_t* d_bad, void* stream) {
    NewBlock blk;
    if (int rc = blk.alloc(narrays, m)) return null_err(rc);
    hipError_t e = gsr::launch_gather_planes(blk.arrays(), scene_stride(m), scene_arrays(d_scene), scene_stride(n),
                                             narrays, (int)sizeof(float), (uint32_t)n, d_indices, (uint32_t)m, d_bad,
                                             blk.get(), static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return null_err(set_err(GSR_E_HIP, "gsr_scene_gather: launch failed: %s", hipGetErrorString(e)));
    return blk.release();
}

extern "C" void* gsr_scene_gather(const void* d_scene, int narrays, int64_t n, const int32_t* d_indices, int64_t m,
                                  uint32_t* d_bad, void* stream) {
    if (!count_in_range(m) || (m > 0 && n == 0))
        return null_err(set_err(GSR_E_ARG, "gsr_scene_gather: m = %lld out of range (n = %lld)", (long long)m, (long long)n));
    if (gsr_scene_bytes(narrays, n) < 0) return nullptr;   // bad narrays or n: the message is set
    if (!d_scene || (m > 0 && !d_indices)) return null_err(set_err(GSR_E_ARG, "gsr_scene_gather: null pointer"));
    if (check_scene_block(d_scene, narrays, n, "gsr_scene_gather") != GSR_OK) return nullptr;
    return scene_gather_checked(d_scene, narrays, n, d_indices, m, d_bad, stream);
}

extern "C" void* gsr_scene_select(const void* d_scene, int narrays, int64_t n, const uint8_t* d_keep, int64_t* m_out,
                                  int32_t* d_indices, void* stream) {
    if (gsr_scene_bytes(narrays, n) < 0) return nullptr;   // bad narrays or n: the message is set
    if (!d_scene || !m_out || (n > 0 && !d_keep)) return null_err(set_err(GSR_E_ARG, "gsr_scene_select: null pointer"));
    if (check_scene_block(d_scene, narrays, n, "gsr_scene_select") != GSR_OK) return nullptr;
    DevBuf<int32_t> own;   // the index list, when the caller gave none
    if (!d_indices && n > 0 && own.alloc((size_t)n)) return nullptr;
    int32_t* idx = d_indices ? d_indices : own.get();
    void* d = nullptr;
    if (gsr_mask_indices(d_keep, n, idx, m_out, stream) == GSR_OK)
        d = scene_gather_checked(d_scene, narrays, n, idx, *m_out, nullptr, stream);
    // the private index list must outlive the gather that reads it
    if (own) (void)hipStreamSynchronize(static_cast<hipStream_t>(stream));
    return d;
}

// ---- scene optimisation (kernel: gsr_scene_adam.hip) ----

extern "C" int gsr_scene_adam_step(void* d_scene, int layout, int64_t n, const gsr_scene_grads* grads,
                                   const gsr_scene_grads* m, const gsr_scene_grads* v, const gsr_adam_config* cfg,
                                   uint32_t* d_bad, void* stream) {
    const char* who = "gsr_scene_adam_step";
    if (!grads || !m || !v || !cfg) return set_err(GSR_E_ARG, "%s: null grads, m, v or cfg", who);
    if (!is_block_layout(layout)) return set_err(GSR_E_ARG, "%s: layout %d is not a scene block", who, layout);
    if (!count_in_range(n)) return set_err(GSR_E_ARG, "%s: n = %lld out of range", who, (long long)n);
    if (n > 0 && !d_scene) return set_err(GSR_E_ARG, "%s: null scene", who);
    const float lrs[9] = {cfg->lr_position, cfg->lr_opacity, cfg->lr_scale, cfg->lr_rot, cfg->lr_sh_dc,
                          cfg->lr_sh_rest, cfg->lr_tcenter, cfg->lr_tscale, cfg->lr_motion};
    for (float lr : lrs)
        if (!std::isfinite(lr) || lr < 0.0f) return set_err(GSR_E_ARG, "%s: a learning rate is negative or not finite", who);
    if (!(cfg->beta1 >= 0.0f && cfg->beta1 < 1.0f) || !(cfg->beta2 >= 0.0f && cfg->beta2 < 1.0f))
        return set_err(GSR_E_ARG, "%s: beta1 = %g, beta2 = %g outside [0, 1)", who, cfg->beta1, cfg->beta2);
    if (!std::isfinite(cfg->eps) || !(cfg->eps > 0.0f)) return set_err(GSR_E_ARG, "%s: eps = %g", who, cfg->eps);
    if (cfg->step < 1) return set_err(GSR_E_ARG, "%s: step = %lld < 1", who, (long long)cfg->step);
    if (cfg->flags & ~(GSR_ADAM_SKIP_ZERO | GSR_ADAM_ZERO_GRADS))
        return set_err(GSR_E_ARG, "%s: unknown flag bits 0x%x", who, cfg->flags);

    // the groups in the block's array order: {gradient, moments, first plane of the pointer,
    // planes, first block array, lr, update kind}
    const bool four_d = layout == GSR_LAYOUT_SCENE_BLOCK_4D;
    const int sh_rest = layout == GSR_LAYOUT_SCENE_BLOCK_SH3 ? GSR_SCENE_SH3_NARRAYS - GSR_A_SH0 - 3
                                                             : GSR_SCENE_NARRAYS - GSR_A_SH0 - 3;
    struct Group {
        float *g, *m, *v;
        int first, planes, array;
        float lr;
        int kind;
        bool temporal;
    };
    const Group groups[9] = {
        {grads->d_position, m->d_position, v->d_position, 0, 3, GSR_A_X, cfg->lr_position, gsr::kAdamPlain, false},
        {grads->d_opacity, m->d_opacity, v->d_opacity, 0, 1, GSR_A_OPACITY, cfg->lr_opacity, gsr::kAdamOpacity, false},
        {grads->d_scale, m->d_scale, v->d_scale, 0, 3, GSR_A_SCALE0, cfg->lr_scale, gsr::kAdamExp, false},
        {grads->d_rot, m->d_rot, v->d_rot, 0, 4, GSR_A_ROT0, cfg->lr_rot, gsr::kAdamPlain, false},
        {grads->d_sh, m->d_sh, v->d_sh, 0, 3, GSR_A_SH0, cfg->lr_sh_dc, gsr::kAdamPlain, false},
        {grads->d_sh, m->d_sh, v->d_sh, 3, sh_rest, GSR_A_SH0 + 3, cfg->lr_sh_rest, gsr::kAdamPlain, false},
        {grads->d_temporal, m->d_temporal, v->d_temporal, 0, 1, GSR_A_TCENTER, cfg->lr_tcenter, gsr::kAdamPlain, true},
        {grads->d_temporal, m->d_temporal, v->d_temporal, 1, 1, GSR_A_TSCALE, cfg->lr_tscale, gsr::kAdamExp, true},
        {grads->d_temporal, m->d_temporal, v->d_temporal, 2, 9, GSR_A_MOTION0, cfg->lr_motion, gsr::kAdamPlain, true},
    };
    gsr::AdamLaunch L{};
    bool skew = misaligned(d_scene, d_bad);
    for (const Group& gr : groups) {
        if (!gr.g || gr.lr == 0.0f) continue;   // frozen: neither read nor written
        if (gr.temporal && !four_d) return set_err(GSR_E_ARG, "%s: d_temporal needs a 4D scene block", who);
        if (!gr.m || !gr.v) return set_err(GSR_E_ARG, "%s: an active group lacks a moment plane", who);
        skew |= misaligned(gr.g, gr.m, gr.v);
        for (int p = 0; p < gr.planes; p++) {
            const int64_t off = (int64_t)(gr.first + p) * n;
            L.plane[L.nplanes++] = gsr::AdamPlane{gr.g + off, gr.m + off, gr.v + off, gr.lr, (uint16_t)(gr.array + p),
                                                  (uint16_t)gr.kind};
        }
    }
    if (L.nplanes == 0) return set_err(GSR_E_ARG, "%s: no active group (a gradient pointer with a non-zero lr)", who);
    if (skew) return set_err(GSR_E_ARG, "%s: misaligned pointer", who);
    if (n == 0) return GSR_OK;
    const double b1 = (double)cfg->beta1, b2 = (double)cfg->beta2, t = (double)cfg->step;
    L.beta1 = cfg->beta1;
    L.beta2 = cfg->beta2;
    L.omb1 = (float)(1.0 - b1);
    L.omb2 = (float)(1.0 - b2);
    L.bc1 = (float)(1.0 - std::pow(b1, t));
    L.bc2 = (float)(1.0 - std::pow(b2, t));
    L.eps = cfg->eps;
    L.flags = cfg->flags;
    HIP_TRY(gsr::launch_scene_adam(scene_arrays(d_scene), scene_stride(n), (uint32_t)n, L, d_bad,
                                   static_cast<hipStream_t>(stream)));
    return GSR_OK;
}

// ---- scene densification (kernels: gsr_scene_densify.hip) ----

extern "C" int gsr_densify_accumulate(const float* d_center, int64_t n, int W, int H, float* d_grad_accum,
                                      uint32_t* d_seen, uint32_t* d_bad, void* stream) {
    const char* who = "gsr_densify_accumulate";
    if (!count_in_range(n)) return set_err(GSR_E_ARG, "%s: n = %lld out of range", who, (long long)n);
    if (W < 1 || H < 1) return set_err(GSR_E_ARG, "%s: %d x %d out of range", who, W, H);
    if (n > 0 && (!d_center || !d_grad_accum || !d_seen)) return set_err(GSR_E_ARG, "%s: null pointer", who);
    if (misaligned(d_center, d_grad_accum, d_seen, d_bad)) return set_err(GSR_E_ARG, "%s: misaligned pointer", who);
    if (n == 0) return GSR_OK;
    HIP_TRY(gsr::launch_densify_accumulate(d_center, (uint32_t)n, W, H, d_grad_accum, d_seen, d_bad,
                                           static_cast<hipStream_t>(stream)));
    return GSR_OK;
}

// The argument errors of gsr_scene_densify's configuration (GSR_OK or GSR_E_ARG with the message set).
static int check_densify_config(const gsr_densify_config& c, const char* who) {
    const float f[5] = {c.grad_threshold, c.scale_split, c.min_opacity, c.prune_scale_max, c.split_shrink};
    for (float x : f)
        if (std::isnan(x)) return set_err(GSR_E_ARG, "%s: a NaN field in the configuration", who);
    if (c.grad_threshold < 0.0f || c.scale_split < 0.0f)
        return set_err(GSR_E_ARG, "%s: grad_threshold = %g or scale_split = %g negative", who, c.grad_threshold,
                       c.scale_split);
    if (c.min_opacity < 0.0f || c.min_opacity > 1.0f)
        return set_err(GSR_E_ARG, "%s: min_opacity = %g outside [0, 1]", who, c.min_opacity);
    if (!(c.prune_scale_max > 0.0f)) return set_err(GSR_E_ARG, "%s: prune_scale_max = %g <= 0", who, c.prune_scale_max);
    if (!std::isfinite(c.split_shrink) || !(c.split_shrink > 1.0f))
        return set_err(GSR_E_ARG, "%s: split_shrink = %g not finite or <= 1", who, c.split_shrink);
    if (c.flags) return set_err(GSR_E_ARG, "%s: unknown flag bits 0x%x", who, c.flags);
    return GSR_OK;
}

extern "C" void* gsr_scene_densify(const void* d_scene, int narrays, int64_t n, const float* d_grad_accum,
                                   const uint32_t* d_seen, const gsr_densify_config* cfg, int32_t* d_src,
                                   uint8_t* d_kind, gsr_densify_report* report, void* stream) {
    const char* who = "gsr_scene_densify";
    if (gsr_scene_bytes(narrays, n) < 0) return nullptr;   // bad narrays or n: the message is set
    if (n > INT32_MAX / 2)
        return null_err(set_err(GSR_E_ARG, "%s: n = %lld > INT32_MAX / 2 (the expansion can double it)", who, (long long)n));
    if (!d_scene || !cfg || !report || (n > 0 && (!d_grad_accum || !d_seen)))
        return null_err(set_err(GSR_E_ARG, "%s: null pointer", who));
    if (check_densify_config(*cfg, who) != GSR_OK) return nullptr;
    if (misaligned(d_grad_accum, d_seen, d_src)) return null_err(set_err(GSR_E_ARG, "%s: misaligned pointer", who));
    if (check_scene_block(d_scene, narrays, n, who) != GSR_OK) return nullptr;

    hipStream_t s = static_cast<hipStream_t>(stream);
    const float* arrays = scene_arrays(d_scene);
    gsr_densify_report rep{};
    DevBuf<uint32_t> counts;   // the chunk counts, their total (n_out), then the four fate totals
    DevBuf<int32_t> own_src;
    DevBuf<uint8_t> own_kind;
    hipError_t e = hipSuccess;
    const uint32_t chunks = n > 0 ? gsr::densify_chunks((uint32_t)n) : 0;
    if (n > 0) {
        if (counts.alloc((size_t)chunks + 5)) return nullptr;
        uint32_t h[5] = {0, 0, 0, 0, 0};
        e = hipMemsetAsync(counts + chunks + 1, 0, 4 * sizeof(uint32_t), s);
        if (e == hipSuccess)
            e = gsr::launch_densify_count(arrays, scene_stride(n), (uint32_t)n, d_grad_accum, d_seen, *cfg, counts,
                                          counts + chunks + 1, s);
        if (e == hipSuccess) e = hipMemcpyAsync(h, counts + chunks, sizeof h, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess)
            return null_err(set_err(GSR_E_HIP, "%s: classification failed: %s", who, hipGetErrorString(e)));
        rep.n_out = h[0];
        rep.kept = h[1];
        rep.cloned = h[2];
        rep.split = h[3];
        rep.pruned = h[4];
        if (rep.kept + rep.cloned + rep.split + rep.pruned != n || rep.n_out != rep.kept + 2 * (rep.cloned + rep.split))
            return null_err(set_err(GSR_E_HIP, "%s: inconsistent expansion counts", who));
    }
    const int64_t m = rep.n_out;
    if (m > 0 && ((!d_src && own_src.alloc((size_t)m)) || (!d_kind && own_kind.alloc((size_t)m)))) return nullptr;
    int32_t* src = d_src ? d_src : own_src.get();
    uint8_t* kind = d_kind ? d_kind : own_kind.get();

    NewBlock blk;
    if (int rc = blk.alloc(narrays, m)) return null_err(rc);
    float* dst = blk.arrays();
    if (m > 0)
        e = gsr::launch_densify_emit(arrays, scene_stride(n), (uint32_t)n, d_grad_accum, d_seen, *cfg, counts,
                                     (uint32_t)m, src, kind, s);
    // the bulk move (and the header, also for m == 0)
    if (e == hipSuccess)
        e = gsr::launch_gather_planes(dst, scene_stride(m), arrays, scene_stride(n), narrays, (int)sizeof(float),
                                      (uint32_t)n, src, (uint32_t)m, nullptr, blk.get(), s);
    if (e == hipSuccess && rep.split > 0)
        e = gsr::launch_densify_split(dst, scene_stride(m), (uint32_t)m, arrays, scene_stride(n), (uint32_t)n, src, kind,
                                      cfg->split_shrink, cfg->seed, s);
    // the scratch and the private lists must outlive the launches that read them
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return null_err(set_err(GSR_E_HIP, "%s: expansion failed: %s", who, hipGetErrorString(e)));
    *report = rep;
    return blk.release();
}

extern "C" void gsr_densify_normals(uint64_t seed, uint32_t index, uint32_t child, float out3[3]) {
    gsr_densify_normal3(seed, index, child, out3);
}

extern "C" int gsr_logf_probe(const float* host_in, int n, float* host_out) {
    if (!host_in || !host_out || n < 0) return set_err(GSR_E_ARG, "gsr_logf_probe: bad argument");
    for (int i = 0; i < n; i++) host_out[i] = gsr_logf(host_in[i]);
    return GSR_OK;
}

extern "C" int gsr_densify_gather_planes(float* d_dst, int64_t dst_stride, const float* d_src_planes,
                                         int64_t src_stride, int nplanes, int64_t n, const int32_t* d_src,
                                         const uint8_t* d_kind, int64_t m, uint32_t* d_bad, void* stream) {
    const char* who = "gsr_densify_gather_planes";
    if (!d_dst || !d_src_planes || !d_src || !d_kind) return set_err(GSR_E_ARG, "%s: null pointer", who);
    if (nplanes < 1) return set_err(GSR_E_ARG, "%s: nplanes = %d < 1", who, nplanes);
    if (!count_in_range(n) || !count_in_range(m) || (m > 0 && n == 0))
        return set_err(GSR_E_ARG, "%s: n = %lld, m = %lld out of range", who, (long long)n, (long long)m);
    if (src_stride < n || dst_stride < m)
        return set_err(GSR_E_ARG, "%s: stride smaller than its count (src %lld < %lld or dst %lld < %lld)", who,
                       (long long)src_stride, (long long)n, (long long)dst_stride, (long long)m);
    if (misaligned(d_dst, d_src_planes, d_src, d_bad)) return set_err(GSR_E_ARG, "%s: misaligned pointer", who);
    HIP_TRY(gsr::launch_densify_gather(d_dst, dst_stride, d_src_planes, src_stride, nplanes, (uint32_t)n, d_src, d_kind,
                                       (uint32_t)m, d_bad, static_cast<hipStream_t>(stream)));
    return GSR_OK;
}

extern "C" int gsr_scene_reset_opacity(void* d_scene, int layout, int64_t n, float cap, float* d_m_opacity,
                                       float* d_v_opacity, void* stream) {
    const char* who = "gsr_scene_reset_opacity";
    if (!is_block_layout(layout)) return set_err(GSR_E_ARG, "%s: layout %d is not a scene block", who, layout);
    if (!count_in_range(n)) return set_err(GSR_E_ARG, "%s: n = %lld out of range", who, (long long)n);
    if (n > 0 && !d_scene) return set_err(GSR_E_ARG, "%s: null scene", who);
    if (!(cap >= GSR_ADAM_OPACITY_MIN && cap <= GSR_ADAM_OPACITY_MAX))
        return set_err(GSR_E_ARG, "%s: cap = %g outside [%g, %g]", who, cap, GSR_ADAM_OPACITY_MIN, GSR_ADAM_OPACITY_MAX);
    if (misaligned(d_scene, d_m_opacity, d_v_opacity)) return set_err(GSR_E_ARG, "%s: misaligned pointer", who);
    if (n == 0) return GSR_OK;
    HIP_TRY(gsr::launch_reset_opacity(scene_arrays(d_scene), scene_stride(n), (uint32_t)n, cap, d_m_opacity,
                                      d_v_opacity, static_cast<hipStream_t>(stream)));
    return GSR_OK;
}

// ---- scene initialisation (kernels: gsr_scene_init.hip) ----

extern "C" int64_t gsr_points_knn_scratch_bytes(int64_t n) {
    if (!count_in_range(n)) return set_err(GSR_E_ARG, "gsr_points_knn_scratch_bytes: n = %lld out of range", (long long)n);
    return gsr::knn_scratch_bytes(n);
}

// The argument errors of a strided [n, 3] array (GSR_OK or GSR_E_ARG with the message set).
static int check_point_strides(int64_t ps, int64_t cs, int64_t n, const char* who, const char* what) {
    if (ps < 1 || cs < 1) return set_err(GSR_E_ARG, "%s: %s stride < 1 (%lld, %lld)", who, what, (long long)ps, (long long)cs);
    // cs <= INT64_MAX / 3 and ps <= INT64_MAX / n keep the products exact; anything larger is
    // no array a device holds
    if (cs > INT64_MAX / 3 || (n > 0 && ps > INT64_MAX / n))
        return set_err(GSR_E_ARG, "%s: %s strides (%lld, %lld) out of range", who, what, (long long)ps, (long long)cs);
    if (ps == cs || !(ps >= 3 * cs || cs >= n * ps))
        return set_err(GSR_E_ARG, "%s: %s strides (%lld, %lld) overlap for n = %lld", who, what, (long long)ps,
                       (long long)cs, (long long)n);
    return GSR_OK;
}

// gsr_points_knn_dist2's argument errors but the scratch's.
static int check_knn_args(const float* d_xyz, int64_t ps, int64_t cs, int64_t n, const float* d_mean2,
                          const uint32_t* d_bad, const char* who) {
    if (!count_in_range(n)) return set_err(GSR_E_ARG, "%s: n = %lld out of range", who, (long long)n);
    if (n > 0 && !d_xyz) return set_err(GSR_E_ARG, "%s: null d_xyz", who);
    if (int rc = check_point_strides(ps, cs, n, who, "point")) return rc;
    if (misaligned(d_xyz, d_mean2, d_bad)) return set_err(GSR_E_ARG, "%s: misaligned pointer", who);
    return GSR_OK;
}

extern "C" int gsr_points_knn_dist2(const float* d_xyz, int64_t point_stride, int64_t comp_stride, int64_t n,
                                    float* d_mean2, uint32_t* d_bad, void* d_scratch, size_t scratch_bytes,
                                    void* stream) {
    const char* who = "gsr_points_knn_dist2";
    if (int rc = check_knn_args(d_xyz, point_stride, comp_stride, n, d_mean2, d_bad, who)) return rc;
    if (n > 0 && (!d_mean2 || !d_scratch)) return set_err(GSR_E_ARG, "%s: null d_mean2 or d_scratch", who);
    if (misaligned(d_scratch)) return set_err(GSR_E_ARG, "%s: misaligned pointer", who);
    const int64_t need = gsr::knn_scratch_bytes(n);
    if ((uint64_t)scratch_bytes < (uint64_t)need)
        return set_err(GSR_E_ARG, "%s: scratch_bytes = %zu, %lld needed", who, scratch_bytes, (long long)need);
    if (n == 0) return GSR_OK;
    HIP_TRY(gsr::launch_points_knn(d_xyz, point_stride, comp_stride, (uint32_t)n, d_mean2, d_bad, d_scratch,
                                   static_cast<hipStream_t>(stream)));
    return GSR_OK;
}

// The argument errors of gsr_scene_from_points' configuration (GSR_OK or GSR_E_ARG with the message set).
static int check_init_config(const gsr_init_config& c, int narrays, const char* who) {
    const float f[6] = {c.opacity, c.min_dist2, c.scale_mul, c.scale_max, c.t_center, c.t_scale};
    for (float x : f)
        if (std::isnan(x)) return set_err(GSR_E_ARG, "%s: a NaN field in the configuration", who);
    if (!(c.opacity >= GSR_ADAM_OPACITY_MIN && c.opacity <= GSR_ADAM_OPACITY_MAX))
        return set_err(GSR_E_ARG, "%s: opacity = %g outside [%g, %g]", who, c.opacity, GSR_ADAM_OPACITY_MIN,
                       GSR_ADAM_OPACITY_MAX);
    if (c.min_dist2 < 0.0f) return set_err(GSR_E_ARG, "%s: min_dist2 = %g < 0", who, c.min_dist2);
    if (!std::isfinite(c.scale_mul) || !(c.scale_mul > 0.0f))
        return set_err(GSR_E_ARG, "%s: scale_mul = %g not finite or <= 0", who, c.scale_mul);
    if (!(c.scale_max > 0.0f)) return set_err(GSR_E_ARG, "%s: scale_max = %g <= 0", who, c.scale_max);
    if (narrays == GSR_SCENE4D_NARRAYS && !(c.t_scale > 0.0f))
        return set_err(GSR_E_ARG, "%s: t_scale = %g <= 0 on a 4D block", who, c.t_scale);
    if (c.flags) return set_err(GSR_E_ARG, "%s: unknown flag bits 0x%x", who, c.flags);
    return GSR_OK;
}

extern "C" void* gsr_scene_from_points(const float* d_xyz, int64_t point_stride, int64_t comp_stride, const float* d_rgb,
                                       int64_t rgb_point_stride, int64_t rgb_comp_stride, int64_t n, int narrays,
                                       const gsr_init_config* cfg, float* d_mean2, uint32_t* d_bad, void* stream) {
    const char* who = "gsr_scene_from_points";
    if (check_knn_args(d_xyz, point_stride, comp_stride, n, d_mean2, d_bad, who) != GSR_OK) return nullptr;
    if (d_rgb && check_point_strides(rgb_point_stride, rgb_comp_stride, n, who, "rgb") != GSR_OK) return nullptr;
    if (misaligned(d_rgb)) return null_err(set_err(GSR_E_ARG, "%s: misaligned pointer", who));
    if (!is_block_narrays(narrays)) return null_err(set_err(GSR_E_ARG, "%s: narrays = %d", who, narrays));
    if (!cfg) return null_err(set_err(GSR_E_ARG, "%s: null cfg", who));
    if (check_init_config(*cfg, narrays, who) != GSR_OK) return nullptr;

    hipStream_t s = static_cast<hipStream_t>(stream);
    // the k-NN scratch, then the statistic when the caller did not ask for it
    const size_t knn_bytes = (size_t)gsr::knn_scratch_bytes(n);
    DevBuf<char> scratch;
    if (n > 0 && scratch.alloc(knn_bytes + (d_mean2 ? 0 : sizeof(float) * (size_t)n))) return nullptr;
    float* mean2 = d_mean2 ? d_mean2 : reinterpret_cast<float*>(scratch.get() + knn_bytes);
    NewBlock blk;
    if (int rc = blk.alloc(narrays, n)) return null_err(rc);
    hipError_t e = gsr::launch_points_knn(d_xyz, point_stride, comp_stride, (uint32_t)n, mean2, d_bad, scratch.get(), s);
    if (e == hipSuccess)
        e = gsr::launch_scene_init_fill(blk.get(), scene_stride(n), narrays, d_xyz, point_stride, comp_stride, d_rgb,
                                        rgb_point_stride, rgb_comp_stride, (uint32_t)n, mean2, *cfg, s);
    // the scratch must outlive the launches that use it
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return null_err(set_err(GSR_E_HIP, "%s failed: %s", who, hipGetErrorString(e)));
    return blk.release();
}

// ---- image loss (kernels: gsr_image_loss.hip) ----

extern "C" int64_t gsr_image_loss_scratch_bytes(int W, int H, int want_grad) {
    if (W < 1 || H < 1 || 3 * (int64_t)W * H > INT32_MAX)
        return set_err(GSR_E_ARG, "gsr_image_loss_scratch_bytes: %d x %d out of range", W, H);
    // the loss slots, then (with a gradient) three partial maps of 3 W H floats
    return 4 * (gsr::kLossSlotFloats + (want_grad ? 9 * (int64_t)W * H : 0));
}

extern "C" int gsr_image_loss(const float* d_image, const float* d_target, int W, int H, const gsr_loss_config* cfg,
                              float* d_grad_image, float* d_loss, void* d_scratch, int64_t scratch_bytes,
                              void* stream) {
    const char* who = "gsr_image_loss";
    if (!d_image || !d_target || !cfg) return set_err(GSR_E_ARG, "%s: null image, target or cfg", who);
    if (!d_grad_image && !d_loss) return set_err(GSR_E_ARG, "%s: neither a gradient nor the loss values asked for", who);
    if (W < 1 || H < 1 || 3 * (int64_t)W * H > INT32_MAX) return set_err(GSR_E_ARG, "%s: %d x %d out of range", who, W, H);
    const float ws[3] = {cfg->w_l1, cfg->w_l2, cfg->w_dssim};
    for (float w : ws)
        if (!std::isfinite(w) || w < 0.0f) return set_err(GSR_E_ARG, "%s: a weight is negative or not finite", who);
    if (ws[0] == 0.0f && ws[1] == 0.0f && ws[2] == 0.0f) return set_err(GSR_E_ARG, "%s: every weight is 0", who);
    if (!std::isfinite(cfg->grad_scale)) return set_err(GSR_E_ARG, "%s: grad_scale = %g", who, cfg->grad_scale);
    if (cfg->flags) return set_err(GSR_E_ARG, "%s: unknown flag bits 0x%x", who, cfg->flags);
    if (!d_scratch) return set_err(GSR_E_ARG, "%s: null scratch", who);
    const int64_t need = gsr_image_loss_scratch_bytes(W, H, d_grad_image != nullptr);
    if (scratch_bytes < need)
        return set_err(GSR_E_ARG, "%s: scratch_bytes = %lld, %lld needed", who, (long long)scratch_bytes, (long long)need);
    if (misaligned(d_image, d_target, d_grad_image, d_loss, d_scratch))
        return set_err(GSR_E_ARG, "%s: misaligned pointer", who);
    if (d_grad_image && (d_grad_image == d_image || d_grad_image == d_target))
        return set_err(GSR_E_ARG, "%s: d_grad_image is d_image or d_target (the gradient launch reads both)", who);

    const double per = (double)cfg->grad_scale / (3.0 * (double)W * (double)H);
    gsr::LossLaunch L{};
    L.w_l1 = (double)cfg->w_l1;
    L.w_l2 = (double)cfg->w_l2;
    L.w_dssim = (double)cfg->w_dssim;
    L.c_l1 = (float)(L.w_l1 * per);
    L.c_l2 = (float)(2.0 * L.w_l2 * per);
    L.c_ssim = (float)(-L.w_dssim * per);
    HIP_TRY(gsr::launch_image_loss(d_image, d_target, W, H, L, d_grad_image, d_loss, static_cast<float*>(d_scratch),
                                   static_cast<hipStream_t>(stream)));
    return GSR_OK;
}

extern "C" void* gsr_scene_upload(const float* host_soa, int64_t n) {
    return gsr_scene_upload_ex(host_soa, GSR_SCENE_NARRAYS, n);
}

extern "C" void gsr_scene_free(void* d) {
    if (d) (void)hipFree(d);
}

extern "C" int gsr_scene_download(const void* d, float* host_soa, int64_t n) {
    if (!d || !host_soa || n < 0) return set_err(GSR_E_ARG, "gsr_scene_download: bad argument");
    gsr_scene_header h{};
    HIP_TRY(hipMemcpy(&h, d, sizeof h, hipMemcpyDeviceToHost));
    const int narrays = (h.narrays == GSR_SCENE4D_NARRAYS || h.narrays == GSR_SCENE_SH3_NARRAYS)
                            ? (int)h.narrays : GSR_SCENE_NARRAYS;
    const int64_t stride = scene_stride(n);
    if (n == 0) return GSR_OK;
    HIP_TRY(hipMemcpy2D(host_soa, sizeof(float) * (size_t)n, scene_arrays(d), sizeof(float) * (size_t)stride,
                        sizeof(float) * (size_t)n, (size_t)narrays, hipMemcpyDeviceToHost));
    return GSR_OK;
}

extern "C" gsr_gaussian* gsr_load_ply_device_ex(const char* filename, int* out_n, int flags, int* out_narrays) {
    int64_t n = -1;
    int is4d = 0;
    int rc = gsr_ply_read_host_ex(filename, nullptr,
                                  (flags & GSR_PLY_SH3) ? GSR_SCENE_SH3_NARRAYS : GSR_SCENE_NARRAYS, 0, &n, flags,
                                  &is4d);
    if (n >= 0 && out_n) *out_n = (int)n;   // misc.cu:38 sets the count before reading data
    if (rc) {
        std::fprintf(stderr, "%s\n", gsr_last_error());
        return nullptr;
    }
    int narrays = (is4d && out_narrays) ? GSR_SCENE4D_NARRAYS : GSR_SCENE_NARRAYS;
    if (flags & GSR_PLY_SH3) narrays = GSR_SCENE_SH3_NARRAYS;   // 3D only (4D properties ignored)
    std::vector<float> soa((size_t)narrays * (size_t)n);
    rc = gsr_ply_read_host_ex(filename, soa.data(), narrays, n, &n, flags, nullptr);
    if (rc) {
        std::fprintf(stderr, "%s\n", gsr_last_error());
        return nullptr;
    }
    void* d = gsr_scene_upload_ex(soa.data(), narrays, n);
    if (!d) std::fprintf(stderr, "CUDA memory allocation failed: %s\n", gsr_last_error());
    if (out_narrays) *out_narrays = narrays;
    return static_cast<gsr_gaussian*>(d);
}

extern "C" gsr_gaussian* gsr_load_ply_device(const char* filename, int* out_n) {
    return gsr_load_ply_device_ex(filename, out_n, 0, nullptr);
}

gsr_gaussian* loadGaussianCudaFromPly(const std::string& filename, int* out_numGaussians) {
    return gsr_load_ply_device(filename.c_str(), out_numGaussians);
}

// gsr_scene_save.cpp — the device side of the scene export (include/gsr.h "scene export"):
// gsr_scene_pack_rows, the stream-ordered pack of a window of a block into .ply rows
// (k_scene_pack, gsr_scene_pack.hip), and gsr_scene_save_ply, which streams a whole block through
// it into a file.  Context-free like gsr_scene.cpp: every call checks its arguments before any
// file or device work.  The file itself (header, temporary name, rename) is gsr_ply.cpp's PlyFile,
// shared with the host writer.
#include <algorithm>

#include "gsr_host.h"

namespace {

constexpr int64_t kDefaultChunkRows = 65536;   // 16.3 MB (3D) or 19.1 MB (4D) per staging buffer

int layout_narrays(int layout) {
    switch (layout) {
    case GSR_LAYOUT_SCENE_BLOCK: return GSR_SCENE_NARRAYS;
    case GSR_LAYOUT_SCENE_BLOCK_4D: return GSR_SCENE4D_NARRAYS;
    case GSR_LAYOUT_SCENE_BLOCK_SH3: return GSR_SCENE_SH3_NARRAYS;
    default: return 0;
    }
}

// One pinned host allocation, freed with its owner.
class PinnedBuf {
public:
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() {
        if (p_) (void)hipHostFree(p_);
    }
    int alloc(size_t bytes) {
        HIP_TRY(hipHostMalloc(&p_, bytes, hipHostMallocDefault));
        return GSR_OK;
    }
    float* get() const { return static_cast<float*>(p_); }

private:
    void* p_ = nullptr;
};

// One event without timing, destroyed with its owner.
class Event {
public:
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    ~Event() {
        if (ev_) (void)hipEventDestroy(ev_);
    }
    int create() {
        HIP_TRY(hipEventCreateWithFlags(&ev_, hipEventDisableTiming));
        return GSR_OK;
    }
    hipEvent_t get() const { return ev_; }

private:
    hipEvent_t ev_ = nullptr;
};

// The two halves of the save's double buffer: a device staging buffer the pack kernel writes, the
// pinned host buffer it is copied into, and the event that marks the copy's end.
struct Stage {
    DevBuf<float> dev;
    PinnedBuf host;
    Event done;
};

// Chunks [0, nchunks) of the block through the two stages into the file.  Everything is ordered
// on `s`: the pack of chunk k follows the copy of chunk k - 2 out of the same staging buffer, and
// the copy of chunk k into a pinned buffer is queued only after the host has written chunk k - 2
// out of it.
int stream_chunks(const void* d_scene, int narrays, int64_t n, int64_t chunk, int P, Stage (&st)[2], gsr::PlyFile& file,
                  hipStream_t s) {
    const int64_t nchunks = (n + chunk - 1) / chunk;
    auto rows_of = [&](int64_t k) { return std::min(chunk, n - k * chunk); };
    auto write_out = [&](int64_t k) -> int {
        HIP_TRY(hipEventSynchronize(st[k & 1].done.get()));
        return file.write(st[k & 1].host.get(), (size_t)rows_of(k) * (size_t)P * sizeof(float));
    };
    for (int64_t k = 0; k < nchunks; k++) {
        Stage& b = st[k & 1];
        const int64_t m = rows_of(k);
        HIP_TRY(gsr::launch_scene_pack(scene_arrays(d_scene), scene_stride(n), narrays, (uint32_t)(k * chunk),
                                       (uint32_t)m, b.dev, s));
        HIP_TRY(hipMemcpyAsync(b.host.get(), b.dev, (size_t)m * (size_t)P * sizeof(float), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipEventRecord(b.done.get(), s));
        if (k > 0)   // the file write of chunk k - 1 runs beside chunk k's pack and copy
            if (int rc = write_out(k - 1)) return rc;
    }
    return write_out(nchunks - 1);
}

}  // namespace

extern "C" int gsr_scene_pack_rows(const void* d_scene, int layout, int64_t n, int64_t first, int64_t count,
                                   float* d_rows, void* stream) {
    const char* who = "gsr_scene_pack_rows";
    const int narrays = layout_narrays(layout);
    if (!narrays) return set_err(GSR_E_ARG, "%s: layout %d is not a scene block", who, layout);
    if (n < 0 || n > INT32_MAX) return set_err(GSR_E_ARG, "%s: n = %lld out of range", who, (long long)n);
    if (first < 0 || count < 0 || first > n || count > n - first)
        return set_err(GSR_E_ARG, "%s: rows [%lld, %lld + %lld) outside [0, %lld)", who, (long long)first,
                       (long long)first, (long long)count, (long long)n);
    if (count > 0 && (!d_scene || !d_rows)) return set_err(GSR_E_ARG, "%s: null pointer", who);
    if ((reinterpret_cast<uintptr_t>(d_scene) | reinterpret_cast<uintptr_t>(d_rows)) % 4)
        return set_err(GSR_E_ARG, "%s: misaligned pointer", who);
    if (count == 0) return GSR_OK;
    HIP_TRY(gsr::launch_scene_pack(scene_arrays(d_scene), scene_stride(n), narrays, (uint32_t)first, (uint32_t)count,
                                   d_rows, static_cast<hipStream_t>(stream)));
    return GSR_OK;
}

extern "C" int gsr_scene_save_ply(const void* d_scene, int narrays, int64_t n, const char* path, int64_t chunk_rows,
                                  void* stream) {
    const char* who = "gsr_scene_save_ply";
    if (!d_scene || !path) return set_err(GSR_E_ARG, "%s: null pointer", who);
    const int64_t P = gsr_ply_row_floats(narrays);
    if (P < 0) return set_err(GSR_E_ARG, "%s: narrays = %d", who, narrays);
    if (n < 0 || n > INT32_MAX) return set_err(GSR_E_ARG, "%s: n = %lld out of range", who, (long long)n);
    if (chunk_rows < 0) return set_err(GSR_E_ARG, "%s: chunk_rows = %lld < 0", who, (long long)chunk_rows);
    if (int rc = check_scene_block(d_scene, narrays, n, who)) return rc;

    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t chunk = std::max<int64_t>(1, std::min(chunk_rows ? chunk_rows : kDefaultChunkRows, n));
    Stage st[2];
    if (n > 0)
        for (Stage& b : st) {
            // a second stage only when there is a second chunk
            if (&b == &st[1] && chunk >= n) break;
            if (int rc = b.dev.alloc((size_t)chunk * (size_t)P)) return rc;
            if (int rc = b.host.alloc((size_t)chunk * (size_t)P * sizeof(float))) return rc;
            if (int rc = b.done.create()) return rc;
        }
    gsr::PlyFile file;
    if (int rc = file.open(path, n, narrays == GSR_SCENE4D_NARRAYS, who)) return rc;
    if (n > 0) {
        const int rc = stream_chunks(d_scene, narrays, n, chunk, (int)P, st, file, s);
        // nothing queued may outlive the stages it writes
        if (rc != GSR_OK) {
            (void)hipStreamSynchronize(s);
            return rc;
        }
    }
    return file.commit();
}

// gsr_scene_pack.hip — the device half of the scene export (include/gsr.h "scene export"): a
// window of a scene block's planes, de-activated, as the interleaved rows of a 3DGS .ply.
#include "gsr_device.h"

namespace gsr {

namespace {

// An SoA -> AoS transposition through the LDS.  A workgroup takes a tile of kPackTileRows = 64
// rows counted from the window's first row, so the tile's output is 64 P contiguous floats
// (15,872 or 18,688 B, a multiple of 256 B) at a 16-B aligned address whenever `rows` is.
//
// Load: the four waves share the P planes (wave w takes properties w, w + 4, ...), lane l is
// row l of the tile.  A plane load is one contiguous 256-B read per wave, and a wave issues all
// of its 16 or 19 before the first use.  Which array a property reads and how it is
// de-activated (PackMap) is uniform per wave: scalar loads from the kernel arguments.  A lane
// past the window's end loads nothing, so [n, stride) of no array is read.
//
// LDS: row l of the tile starts at word l S, S = P | 1.  The ds_write_b32 of one property puts
// lane l on bank (l S + p) % 32 within its 32-lane half: with P = 62 lanes l and l + 16 would
// share a bank (62 * 16 = 31 * 32), with an odd S the 32 lanes cover the 32 banks.  P = 73 is
// odd already, so its tile is the output image itself and is read back as ds_read_b128; the 62
// tile has one pad word per row and is read back word by word (four ds_read_b32 per 16-B store,
// lanes 8 apart on one bank: 4 LDS cycles each, about a quarter of the tile's 62 write cycles
// again and two orders under its 32 KB of memory traffic).
//
// Store: thread t writes output words 4t .. 4t + 3 (+ 1,024 per round) as one 16-B store, a wave
// 1 KiB contiguous; the last tile's partial group of four goes word by word.  A `rows` that is
// only 4-B aligned takes 4-B stores, a wave's 256 B contiguous.  Nothing at or past count * P
// is written.
constexpr int kPackThreads = 256;
constexpr int kPackWaves = kPackThreads / 64;

template <int P>
__global__ __launch_bounds__(kPackThreads) void k_scene_pack(const float* __restrict__ arrays, int64_t stride,
                                                              uint32_t first, uint32_t count,
                                                              float* __restrict__ rows, const PackMap map) {
    constexpr int S = P | 1;
    constexpr int PER = (P + kPackWaves - 1) / kPackWaves;
    __shared__ __attribute__((aligned(16))) float tile[kPackTileRows * S];

    // count <= INT32_MAX: row0 + 64 stays under 2^32
    const uint32_t row0 = blockIdx.x * (uint32_t)kPackTileRows;
    const uint32_t m = min(count - row0, (uint32_t)kPackTileRows);
    const uint32_t lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const bool live = lane < m;
    const float* __restrict__ src = arrays + ((int64_t)first + row0 + lane);

    float v[PER];
#pragma unroll
    for (int i = 0; i < PER; i++) {
        const int p = wave + i * kPackWaves;
        v[i] = 0.0f;
        if (p < P && live && map.kind[p] != kPackZero) v[i] = src[(int64_t)map.array[p] * stride];
    }
#pragma unroll
    for (int i = 0; i < PER; i++) {
        const int p = wave + i * kPackWaves;
        if (p >= P) break;
        const int kind = map.kind[p];
        float x = v[i];
        if (kind == kPackLog) x = gsr_raw_log(x);
        else if (kind == kPackLogit) x = gsr_raw_logit(x);
        tile[lane * S + p] = x;
    }
    __syncthreads();

    const uint32_t words = m * (uint32_t)P;
    float* __restrict__ out = rows + (int64_t)row0 * P;
    auto at = [&](uint32_t j) { return tile[j + (j / (uint32_t)P) * (uint32_t)(S - P)]; };
    if ((reinterpret_cast<uintptr_t>(rows) & 15u) == 0) {
        for (uint32_t j = threadIdx.x * 4u; j < words; j += kPackThreads * 4u) {
            if (j + 4u <= words) {
                float4 q;
                if (S == P) q = *reinterpret_cast<const float4*>(&tile[j]);
                else q = make_float4(at(j), at(j + 1u), at(j + 2u), at(j + 3u));
                *reinterpret_cast<float4*>(out + j) = q;
            } else {
                for (uint32_t k = j; k < words; k++) out[k] = at(k);
            }
        }
    } else {
        for (uint32_t j = threadIdx.x; j < words; j += kPackThreads) out[j] = at(j);
    }
}

}  // namespace

hipError_t launch_scene_pack(const float* arrays, int64_t stride, int narrays, uint32_t first, uint32_t count,
                             float* rows, hipStream_t s) {
    if (count == 0) return hipSuccess;
    const PackMap map = pack_map(narrays);
    const dim3 grid((uint32_t)grid_for(count, kPackTileRows));
    if (map.nprops == 62)
        hipLaunchKernelGGL(k_scene_pack<62>, grid, dim3(kPackThreads), 0, s, arrays, stride, first, count, rows, map);
    else if (map.nprops == 73)
        hipLaunchKernelGGL(k_scene_pack<73>, grid, dim3(kPackThreads), 0, s, arrays, stride, first, count, rows, map);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace gsr

// gsr_geom_device.h — device helpers that cross the geometry stages of the gfx950 kernels
// (gsr_kernels.hip, gsr_bucket_sort.hip): the tile-rectangle format the preprocess writes and
// the sorts and the binning read, and the tile rank the bucket sort's local kernels and both
// binning scatters share.  Inline functions and constants only: no kernels, no __constant__
// data.  What every kernel file shares is in gsr_device.h.
#pragma once

#include "gsr_device.h"

namespace gsr {

namespace {

// Compact tile rectangle of one Gaussian for the emission: tx0 | tx1 << 16 |
// ty0 << 32 | ty1 << 48; tile count (tx1 - tx0 + 1) * (ty1 - ty0 + 1), which
// is 0 for the dead value below (tx0 = ty0 = 1, tx1 = ty1 = 0).
constexpr uint64_t kDeadRect = 0x0000000100000001ull;
__device__ __forceinline__ uint32_t rect_count(uint64_t r) {
    const int tx0 = (int)(r & 0xffffu), tx1 = (int)((r >> 16) & 0xffffu);
    const int ty0 = (int)((r >> 32) & 0xffffu), ty1 = (int)(r >> 48);
    return (uint32_t)((tx1 - tx0 + 1) * (ty1 - ty0 + 1));
}

// 4-B form of a tile rectangle for grids of at most 256 tiles per axis (the
// binning path): tx0 | tx1 << 8 | ty0 << 16 | ty1 << 24.  Lossless there (every
// coordinate is < 256; the dead value packs to 0x00010001 and unpacks to kDeadRect).
__device__ __forceinline__ uint32_t pack_rect(uint64_t r) {
    return (uint32_t)(r & 0xffu) | (uint32_t)((r >> 8) & 0xff00u) | (uint32_t)((r >> 16) & 0xff0000u) |
           (uint32_t)((r >> 24) & 0xff000000u);
}
__device__ __forceinline__ uint64_t unpack_rect(uint32_t p) {
    return (uint64_t)(p & 0xffu) | ((uint64_t)((p >> 8) & 0xffu) << 16) | ((uint64_t)((p >> 16) & 0xffu) << 32) |
           ((uint64_t)(p >> 24) << 48);
}

__device__ __forceinline__ uint32_t rect_rows(uint64_t r) {
    return rect_count(r) ? (uint32_t)((r >> 48) - ((r >> 32) & 0xffffu) + 1u) : 0u;
}
__device__ __forceinline__ uint32_t rect_cols(uint64_t r) {
    return rect_count(r) ? (uint32_t)(((r >> 16) & 0xffffu) - (r & 0xffffu) + 1u) : 0u;
}

// Stable rank of one tile of up to 256*ITEMS items with BITS-bit digits.  Item
// k of thread t is tile element w*64*ITEMS + k*64 + lane (each wave's items are
// contiguous).  On return pos[k] is the item's slot in the digit-sorted tile,
// s_lbase[d] the first slot of digit d; returns the tile's count of digit t.
// Per k-slot every lane reads its digit's running wave count and the slot's
// leader of each digit ADDS the slot's count (ds_add, no return): LDS ops of a
// wave execute in issue order, so slot k's read sees slots < k and nothing waits
// on a read before the next slot is issued.
template <int ITEMS, int BITS, bool RA>
__device__ __forceinline__ uint32_t bin_rank_tile(const uint32_t (&dig)[ITEMS], uint32_t tn,
                                                  uint32_t (&pos)[ITEMS], uint32_t (*s_wc)[256],
                                                  uint32_t* s_lbase, uint32_t* s_scr) {
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    const uint64_t lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
#pragma unroll
    for (int k = 0; k < 4; k++) s_wc[k][t] = 0;
    __syncthreads();
    if (RA) {
#pragma unroll
        for (int k = 0; k < ITEMS; k++) {
            const uint32_t el = w * 64 * ITEMS + k * 64 + lane;
            pos[k] = el < tn ? atomicAdd(&s_wc[w][dig[k]], 1u) : 0u;
        }
    } else {
        uint32_t before[ITEMS], inslot[ITEMS];
#pragma unroll
        for (int k = 0; k < ITEMS; k++) {
            const uint32_t el = w * 64 * ITEMS + k * 64 + lane;
            const bool valid = el < tn;
            const uint32_t d = dig[k];
            const uint64_t peers = match_peers<BITS>(d, valid, BITS);
            inslot[k] = (uint32_t)__popcll(peers & lt_mask);
            before[k] = s_wc[w][d];
            if (valid && (uint32_t)(__ffsll((unsigned long long)peers) - 1) == lane)
                atomicAdd(&s_wc[w][d], (uint32_t)__popcll(peers));
        }
#pragma unroll
        for (int k = 0; k < ITEMS; k++) pos[k] = before[k] + inslot[k];
    }
    __syncthreads();
    uint32_t tcount;
    {
        // each wave's first slot of digit t, tile base included (s_wc[w][t] = s_lbase[t] +
        // the earlier waves' counts), so an item reads one word for its slot, not two
        const uint32_t c0 = s_wc[0][t], c1 = s_wc[1][t], c2 = s_wc[2][t], c3 = s_wc[3][t];
        tcount = c0 + c1 + c2 + c3;
        uint32_t tot;
        const uint32_t lb = block_exclusive_scan<uint32_t>(tcount, s_scr, tot);   // barriers: reads done
        s_lbase[t] = lb;
        s_wc[0][t] = lb;
        s_wc[1][t] = lb + c0;
        s_wc[2][t] = lb + c0 + c1;
        s_wc[3][t] = lb + c0 + c1 + c2;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < ITEMS; k++) {
        const uint32_t el = w * 64 * ITEMS + k * 64 + lane;
        if (el < tn) pos[k] += s_wc[w][dig[k]];
    }
    return tcount;
}

}  // namespace

}  // namespace gsr

// gsr_bucket_sort.hip — the bucket depth sort of the gfx950 (CDNA4) 3DGS rasterizer's binning
// path (GSR_TUNE_DEPTH_BUCKETS; DESIGN.md sections 3 and 9): count, scan, scatter, the local
// sorts (small and big buckets) with the fused row-pass count, and the splitters.  Shared wave /
// workgroup helpers: gsr_device.h; the tile-rectangle format and bin_rank_tile: gsr_geom_device.h.
#include "gsr_device.h"
#include "gsr_geom_device.h"

namespace gsr {

namespace {

// ------------------------------------------------------------------ bucket depth sort
//
// The binning path's global depth sort in two global steps instead of three or four
// LSD passes (GSR_TUNE_DEPTH_BUCKETS).  Stable order of (depth key, index), exactly
// the LSD passes' order:
//   k_bkt_count    per workgroup chunk, the histogram over B buckets: bucket(key) =
//                  the number of splitters <= key (B - 1 sorted splitters in LDS; the
//                  last is 0xFFFFFFFF, so bucket B - 1 holds exactly the keys equal to
//                  0xFFFFFFFF: culled items and saturated live keys, which tie)
//   k_bkt_scan     per bucket, exclusive scan over the chunks (a chunk-major histogram:
//                  every access a coalesced row segment); k_bkt_scan_g for the big kind
//   k_bkt_scatter  stable scatter of the preprocess order into the buckets (per-wave
//                  returning LDS atomics on packed 16-bit counters, so the rank of an
//                  item is its order among the wave's earlier items of its bucket);
//                  every item lands at its bucket's range, index-ordered inside it; the
//                  tile rects ride along as payloads
//   k_bkt_local    one workgroup per live bucket: load it (<= kBktCap items), stable
//                  LSD in LDS over the bits (key - bucket min) spans (typically 11 on
//                  config 2: two 8-bit passes), write it back in place.  A bucket over
//                  capacity is sorted by the same workgroup through global memory
//                  (stable 8-bit passes ping-ponging with the scratch buffer), so any
//                  splitters give the exact order; they only set the speed
// Two kinds ship (gsr_runtime.cpp bkt_big).  Small (up to 2M items, B = 256..4,096 by size):
// k_bkt_count, k_bkt_scan, the unstaged k_bkt_scatter (16-B records, its own splitter search),
// k_bkt_local.  Big (above 2M, B = kBigBuckets): k_bkt_count handing each item's bucket on,
// k_bkt_scan_g, the staged k_bkt_scatter (12-B records), k_bbk_local, then k_bkt_local for the
// buckets k_bbk_local left.
// Splitters are the previous frame's quantiles: k_bkt_local writes the key at each
// bkt_split_pos of the live order for the next frame (double-buffered; the open first and
// last live buckets a quarter share, the rest even), so the buckets hold about n / B
// items each while the camera moves smoothly.  A context's
// first frame runs the LSD passes and k_bkt_splitters takes the quantiles from them.
// Stability: the scatter keeps index order inside a bucket, the local passes are stable
// and buckets are key ranges in order, so ties stay in index order — the same order as
// render.cu's CUB SortPairs of (tile << 32 | depth) within each tile (render.cu:1099-1118).
constexpr int kBktThreads = 256;
constexpr int kBktItems = 8;                                  // items per thread per tile
constexpr uint32_t kBktTile = kBktThreads * kBktItems;        // 2048
constexpr uint32_t kBktCap = kBktTile;                        // local sort capacity (items)
static_assert(kBktCap == kMaxBucketCap && kMaxBuckets == 4096, "gsr_internal.h bucket sort limits");

// The splitters in LDS as an implicit search tree in breadth-first (Eytzinger) order:
// node i at depth d, position p = i + 1 - 2^d holds the sorted splitter of rank
// (2p + 1) 2^(h - 1 - d) - 1 (h = log2 B; the B - 1 splitters fill the tree exactly).  Each
// search step reads one tree level, and a level's nodes are consecutive words.  (The plain
// sorted array put every address of the first search steps on ONE LDS bank -- b + st - 1
// with b a multiple of 2 st -- up to 32-way conflicts: the count kernel took 10 us.)
template <int B, int TH = kBktThreads>
__device__ __forceinline__ void bkt_load_splitters(uint32_t* s_T, const uint32_t* __restrict__ splitters) {
    // B / TH nodes per thread, every load issued before the first LDS write: a rolled
    // loop waited for each load in turn (four serial memory round trips at B = 1,024)
    static_assert(B >= TH, "one node per thread at least");
    constexpr int h = __builtin_ctz(B);
    constexpr int kPer = B / TH;
    uint32_t v[kPer], jj[kPer];
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const uint32_t i = threadIdx.x + (uint32_t)k * TH;
        const int d = 31 - __clz((int)(i + 1u));
        const uint32_t p = i + 1u - (1u << d);
        const int sh = h - 1 - d;                               // < 0 only for i = B - 1 (no node)
        jj[k] = sh >= 0 ? ((2u * p + 1u) << sh) - 1u : (uint32_t)B - 2u;   // sorted rank
        v[k] = splitters[min(jj[k], (uint32_t)B - 3u)];
    }
#pragma unroll
    for (int k = 0; k < kPer; k++)
        s_T[threadIdx.x + (uint32_t)k * TH] = jj[k] < (uint32_t)B - 2u ? v[k] : 0xffffffffu;
}

// The buckets of N keys: bucket(key) = the number of the B - 1 sorted splitters that are
// <= key (the last is 0xFFFFFFFF, so a key 0xFFFFFFFF lands in bucket B - 1), by a walk
// down the tree of bkt_load_splitters.  Level by level, so each level's N LDS reads are in
// flight together.
template <int B, int N>
__device__ __forceinline__ void bkt_of_n(const uint32_t* s_T, const uint32_t (&key)[N], uint32_t (&bk)[N]) {
#pragma unroll
    for (int k = 0; k < N; k++) bk[k] = 0;
#pragma unroll
    for (int lvl = 0; lvl < __builtin_ctz(B); lvl++) {
        uint32_t v[N];
#pragma unroll
        for (int k = 0; k < N; k++) v[k] = s_T[bk[k]];
#pragma unroll
        for (int k = 0; k < N; k++) bk[k] = 2u * bk[k] + (v[k] <= key[k] ? 2u : 1u);
    }
#pragma unroll
    for (int k = 0; k < N; k++) bk[k] -= (uint32_t)B - 1u;
}

template <int B>
__global__ __launch_bounds__(kBktThreads) void k_bkt_count(const uint64_t* __restrict__ in, uint32_t n,
                                                           const uint32_t* __restrict__ splitters, int groups,
                                                           uint32_t* __restrict__ hist,
                                                           uint16_t* __restrict__ bid = nullptr) {
    GSR_GEOM_PRIO();
    __shared__ uint32_t s_S[B], s_h[B];
    const uint32_t t = threadIdx.x, lane = t & 63u;
    uint64_t b, e;
    chunk_range(n, groups, blockIdx.x, kBktTile, b, e);
    uint32_t key[kBktItems];
    auto load = [&](uint64_t i0, uint32_t (&kk)[kBktItems]) {
#pragma unroll
        for (int k = 0; k < kBktItems; k++) {
            const uint64_t i = i0 + (uint64_t)k * kBktThreads + t;
            kk[k] = i < e ? (uint32_t)(in[i] >> 32) : 0xffffffffu;
        }
    };
    load(b, key);   // the first tile's keys travel together with the splitters: one memory round trip
    bkt_load_splitters<B>(s_S, splitters);
    for (uint32_t j = t; j < (uint32_t)B; j += kBktThreads) s_h[j] = 0;
    __syncthreads();
    uint32_t dead = 0;   // culled items all share the last bucket: counted by ballots, not 64-way atomics
    for (uint64_t i0 = b; i0 < e; i0 += kBktTile) {
        // the next tile's keys are in flight while this tile walks the tree (scenes above
        // 1M items give a workgroup several tiles)
        uint32_t nkey[kBktItems];
        if (i0 + kBktTile < e) load(i0 + kBktTile, nkey);
        uint32_t bk[kBktItems];
        bkt_of_n<B>(s_S, key, bk);
#pragma unroll
        for (int k = 0; k < kBktItems; k++) {
            const uint64_t i = i0 + (uint64_t)k * kBktThreads + t;
            const bool d = key[k] == 0xffffffffu;
            dead += (uint32_t)__popcll(__ballot(d && i < e));
            if (!d) atomicAdd(&s_h[bk[k]], 1u);
            if (bid && i < e) bid[i] = (uint16_t)bk[k];   // the scatter reads it instead of searching again
        }
        if (i0 + kBktTile < e) {
#pragma unroll
            for (int k = 0; k < kBktItems; k++) key[k] = nkey[k];
        }
    }
    if (lane == 0 && dead) atomicAdd(&s_h[B - 1], dead);
    __syncthreads();
    // chunk-major (hist[chunk][bucket]): this workgroup's row is one coalesced 4B-per-bucket run
    // (bucket-major, each of its B words went to another cache line: 15 us for 1M items)
    for (uint32_t j = t; j < (uint32_t)B; j += kBktThreads) hist[(size_t)blockIdx.x * B + j] = s_h[j];
}

// Per bucket, the exclusive scan over the chunks of the chunk-major histogram (in place)
// and the bucket's total.  64 buckets per workgroup (one per lane), 16 waves splitting the
// chunks: every load is a coalesced 256-B row segment.  groups <= kBktMaxGroups.
constexpr int kBktMaxGroups = kMaxBucketGroups;
template <int B>
__global__ __launch_bounds__(1024) void k_bkt_scan(uint32_t* __restrict__ hist, int groups,
                                                   uint32_t* __restrict__ totals) {
    GSR_GEOM_PRIO();
    constexpr int kPerMax = kBktMaxGroups / 16;
    __shared__ uint32_t s_part[16][64];
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    const uint32_t b = blockIdx.x * 64u + lane;
    const uint32_t per = ((uint32_t)groups + 15u) / 16u;
    const uint32_t g0 = w * per;
    uint32_t v[kPerMax], sum = 0;
#pragma unroll
    for (int i = 0; i < kPerMax; i++) {
        const uint32_t g = g0 + (uint32_t)i;
        v[i] = (uint32_t)i < per && g < (uint32_t)groups ? hist[(size_t)g * B + b] : 0u;
        sum += v[i];
    }
    s_part[w][lane] = sum;
    __syncthreads();
    uint32_t run = 0, tot = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) {
        const uint32_t p = s_part[k][lane];
        run += k < w ? p : 0u;
        tot += p;
    }
    if (w == 0) totals[b] = tot;
    // the frame's "a live item has key 0xFFFFFFFF" word (bkt_sat_word), raised by the scatter
    if (blockIdx.x == 0 && t == 0) totals[2 * B + 1] = 0u;
#pragma unroll
    for (int i = 0; i < kPerMax; i++) {
        const uint32_t g = g0 + (uint32_t)i;
        if ((uint32_t)i < per && g < (uint32_t)groups) {
            hist[(size_t)g * B + b] = run;
            run += v[i];
        }
    }
}

// The big buckets' scan (kBigBuckets buckets, up to kBigBucketGroups chunks: k_bkt_scan's
// layout put 1.25 MB through 8 workgroups, 23 us at 611 chunks): 16 buckets per 1,024-thread
// workgroup, each wave's four 16-lane quarters reading a 64-B row segment of four different
// chunks (64 chunk slices per workgroup), the slices' sums combined in LDS.  B / 16
// workgroups.  (A wave per bucket measured 8.5 against 5.9 us)
__global__ __launch_bounds__(1024) void k_bkt_scan_g(uint32_t* __restrict__ hist, int groups,
                                                     uint32_t* __restrict__ totals) {
    GSR_GEOM_PRIO();
    constexpr int B = kBigBuckets;
    constexpr int kPerMax = (kBigBucketGroups + 63) / 64;
    __shared__ uint32_t s_part[64][16];
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    const uint32_t bl = lane & 15u, sl = w * 4u + (lane >> 4);   // bucket in the group, chunk slice
    const uint32_t b = blockIdx.x * 16u + bl;
    const uint32_t per = ((uint32_t)groups + 63u) / 64u;
    const uint32_t g0 = sl * per;
    uint32_t v[kPerMax], sum = 0;
#pragma unroll
    for (int i = 0; i < kPerMax; i++) {
        const uint32_t g = g0 + (uint32_t)i;
        v[i] = (uint32_t)i < per && g < (uint32_t)groups ? hist[(size_t)g * B + b] : 0u;
        sum += v[i];
    }
    s_part[sl][bl] = sum;
    __syncthreads();
    uint32_t run = 0, tot = 0;
    for (uint32_t k = 0; k < 64u; k++) {
        const uint32_t p = s_part[k][bl];
        run += k < sl ? p : 0u;
        tot += p;
    }
    if (sl == 0) totals[b] = tot;
    if (blockIdx.x == 0 && t == 0) totals[2 * B + 1] = 0u;   // bkt_sat_word (as k_bkt_scan)
#pragma unroll
    for (int i = 0; i < kPerMax; i++) {
        const uint32_t g = g0 + (uint32_t)i;
        if ((uint32_t)i < per && g < (uint32_t)groups) {
            hist[(size_t)g * B + b] = run;
            run += v[i];
        }
    }
}

// 16-bit half h of the packed counter word v.
__device__ __forceinline__ uint32_t half16(uint32_t v, uint32_t h) { return (v >> (16u * h)) & 0xffffu; }

// Bucket records: 16 B {index, key, rect, 0} (R12 false: one store request per item in the
// unstaged scatter), or 12 B {index, key, rect} (R12: the staged scatter writes runs, where
// the bytes, not the requests, bound it; a quarter fewer of them).
struct __attribute__((packed, aligned(4))) BktRec12 {
    uint32_t i, k, r;
};
template <bool R12>
__device__ __forceinline__ uint4 rec_get(const uint4* __restrict__ rec, uint32_t q) {
    if (R12) {
        const BktRec12 v = reinterpret_cast<const BktRec12*>(rec)[q];
        return make_uint4(v.i, v.k, v.r, 0u);
    }
    return rec[q];
}
template <bool R12>
__device__ __forceinline__ void rec_put(uint4* __restrict__ rec, uint32_t q, uint32_t i, uint32_t k, uint32_t r) {
    if (R12) reinterpret_cast<BktRec12*>(rec)[q] = BktRec12{i, k, r};
    else rec[q] = make_uint4(i, k, r, 0u);
}

// bstart (B + 2 words): written by chunk 0's workgroup, the first position of every bucket
// and bstart[B] = n (k_bkt_local reads its bucket's range there); bstart[B + 1] (cleared by
// k_bkt_scan) is raised when a live item (a tile rect that covers tiles) has key 0xFFFFFFFF.
// TH threads (512 from 512 buckets up: twice the waves of 256, half the items per wave, so
// each wave's latency chain is half as long; the grid is only ~n / 2,048 workgroups:
// 16.3-16.8 -> 15.6-15.8 us at config 2, profiles/r05_kt_bkt_scatter512.txt).
// Live items go out as one 16-B record {index, key, rect, 0} into rec (one store request per
// item: a 4,096-way scatter writes ~one item per bucket per tile, so every store of a wave hits
// its own cache line and the scatter is bound by the L2's request rate, not by bytes: two
// arrays, item and rect, were two requests per item); k_bkt_local reads a bucket's records
// back contiguously.  The last bucket (key 0xFFFFFFFF, never sorted) goes straight to its
// final place in out / pay_out.  The next tile's items and rects are loaded while this one
// is ranked.
// STAGED (the big buckets' scatter): the tile is laid out in LDS by bucket first (tile-local
// position = the bucket's offset in the tile + the item's stable rank in it), then written out
// by position, so the lanes of a store that hold items of one bucket write consecutive 12-B
// records (a run per bucket and tile: ~4 items at 512 buckets) instead of one store request
// each.  It takes every item's bucket from the count kernel (bid) instead of searching the
// splitters again, and thread t < B / 2 owns counter word t (buckets 2t, 2t + 1), so the
// word's wave prefix and the tile offsets' scan are one step; the counters are cleared for the
// next tile after their last read (the stage writes), so a tile starts without a clear +
// barrier: five barriers per tile.  Unstaged (the small kind): the scatter searches the
// splitters itself and writes one 16-B record per item straight from registers.
template <int B, bool RA, int TH, bool STAGED>
__global__ __launch_bounds__(TH) __attribute__((amdgpu_waves_per_eu(1))) void k_bkt_scatter(const uint64_t* __restrict__ in,
                                                             uint64_t* __restrict__ out, uint32_t n,
                                                             const uint32_t* __restrict__ splitters, int groups,
                                                             const uint32_t* __restrict__ hist,
                                                             const uint32_t* __restrict__ totals,
                                                             const uint32_t* __restrict__ rect,
                                                             uint32_t* __restrict__ pay_out,
                                                             uint32_t* __restrict__ bstart,
                                                             uint4* __restrict__ rec,
                                                             const uint16_t* __restrict__ bid) {
    GSR_GEOM_PRIO();
    constexpr uint32_t TILE = kBktTile;
    constexpr int NW = TH / 64, kIt = TILE / TH;  // waves; items per thread
    constexpr uint32_t kW = B / 2;                      // packed counter words per wave
    constexpr int kPer = B / TH;                        // buckets per thread (scan)
    constexpr int kWPer = (kW + TH - 1) / TH;           // counter words per thread
    static_assert(kPer >= 1 && kIt * TH == TILE, "bucket / thread split");
    static_assert(!STAGED || B / 2 <= TH, "staged: one counter word per thread");
    __shared__ uint32_t s_S[B], s_gbase[B];
    __shared__ uint32_t s_wc[NW][kW];
    __shared__ uint32_t s_scr[NW];
    // STAGED: per-bucket tile offsets, the tile in bucket order
    __shared__ uint32_t s_tp[STAGED ? B : 1];
    __shared__ uint4 s_stage[STAGED ? TILE : 1];
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    const uint64_t lt_mask = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    const int chunk = xcd_chunk((int)blockIdx.x, groups);   // each XCD takes a contiguous run of chunks
    uint64_t b, e;
    chunk_range(n, groups, chunk, kBktTile, b, e);   // chunks as k_bkt_count's
    const uint32_t wbase = w * 64 * kIt;
    uint64_t it[kIt];
    uint32_t pv[kIt], bv[kIt];
    // STAGED: the count kernel's bucket of every item (bid), loaded with the tile
    auto load = [&](uint64_t tb, uint32_t tn, uint64_t (&ii)[kIt], uint32_t (&pp)[kIt], uint32_t (&bb)[kIt]) {
#pragma unroll
        for (int k = 0; k < kIt; k++) {
            const uint32_t el = wbase + k * 64 + lane;
            ii[k] = el < tn ? in[tb + el] : ~0ull;
            pp[k] = el < tn ? rect[tb + el] : 0u;   // the input is the preprocess order: rect by position
            if (STAGED) bb[k] = el < tn ? (uint32_t)bid[tb + el] : (uint32_t)B - 1u;
        }
    };
    // the first tile's items and rects, the splitters, the bucket totals and this chunk's
    // histogram row are all loaded in one memory round trip
    load(b, (uint32_t)min((uint64_t)TILE, e - b), it, pv, bv);
    if (!STAGED) bkt_load_splitters<B, TH>(s_S, splitters);
    {   // this chunk's first slot in every bucket: the bucket's start + the earlier chunks' items
        uint32_t loc[kPer], hrow[kPer], sum = 0;
#pragma unroll
        for (int k = 0; k < kPer; k++) {
            loc[k] = totals[t * kPer + k];
            hrow[k] = hist[(size_t)chunk * B + t * kPer + k];
            sum += loc[k];
        }
        uint32_t tot;
        uint32_t run = block_exclusive_scan<uint32_t, NW>(sum, s_scr, tot);
#pragma unroll
        for (int k = 0; k < kPer; k++) {
            const uint32_t d = t * kPer + k;
            if (chunk == 0) bstart[d] = run;
            s_gbase[d] = run + hrow[k];
            run += loc[k];
        }
        if (chunk == 0 && t == 0) bstart[B] = n;
    }
    if (b >= e) return;   // uniform per workgroup, after the scan's barriers
    if (STAGED) {   // the first tile's counter clear; every later one follows the stage writes
        for (uint32_t j = t; j < NW * kW; j += TH) (&s_wc[0][0])[j] = 0;
        __syncthreads();
    }
    for (uint64_t tb = b; tb < e; tb += TILE) {
        const uint32_t tn = (uint32_t)min((uint64_t)TILE, e - tb);
        const bool more = tb + TILE < e;   // uniform
        uint64_t nit[kIt];
        uint32_t npv[kIt], nbv[kIt];
        if (more) load(tb + TILE, (uint32_t)min((uint64_t)TILE, e - tb - TILE), nit, npv, nbv);
        if (!STAGED) {
            for (uint32_t j = t; j < NW * kW; j += TH) (&s_wc[0][0])[j] = 0;
            __syncthreads();
        }
        uint32_t dg[kIt], rk[kIt], keys[kIt];
#pragma unroll
        for (int k = 0; k < kIt; k++) keys[k] = (uint32_t)(it[k] >> 32);
        if (STAGED) {
#pragma unroll
            for (int k = 0; k < kIt; k++) dg[k] = bv[k];
        } else {
            bkt_of_n<B>(s_S, keys, dg);   // a key 0xFFFFFFFF (culled) counts every splitter: bucket B - 1
        }
        // culled items (the last bucket) rank by ballot against a running wave count, so the
        // live items' returning atomics have no LDS read between them and stay in flight together
        uint32_t dead_run = 0;
        uint32_t old[kIt];
#pragma unroll
        for (int k = 0; k < kIt; k++) {
            const uint32_t el = wbase + k * 64 + lane;
            const bool valid = el < tn;
            const bool dead = keys[k] == 0xffffffffu;
            const uint32_t d = dg[k];
            // a live Gaussian whose key saturated (depth >= ~4295 under a far clip that keeps
            // it) shares the last bucket with the culled items: k_bkt_local's fused row count
            // must then bin that bucket too (rare: a plain vector store of 1)
            if (valid && dead && rect_count(unpack_rect(pv[k]))) bstart[B + 1] = 1u;
            const uint64_t dm = __ballot(valid && dead);
            uint32_t r = dead_run + (uint32_t)__popcll(dm & lt_mask);
            dead_run += (uint32_t)__popcll(dm);
            const uint32_t sh = 16u * (d & 1u);
            if (RA) {
                // every lane adds (0 when it has no live item): no branch, so the eight returning
                // atomics are in flight together; the halves are taken after the loop
                old[k] = atomicAdd(&s_wc[w][d >> 1], valid && !dead ? 1u << sh : 0u);
            } else {
                const uint64_t peers = match_peers<12>(d, valid && !dead, 12);   // every lane takes part
                if (valid && !dead) {
                    r = half16(s_wc[w][d >> 1], d & 1u) + (uint32_t)__popcll(peers & lt_mask);
                    if (lane == (uint32_t)(__ffsll((unsigned long long)peers) - 1))
                        atomicAdd(&s_wc[w][d >> 1], (uint32_t)__popcll(peers) << sh);
                }
            }
            rk[k] = r;
        }
        if (RA) {
#pragma unroll
            for (int k = 0; k < kIt; k++)
                if (keys[k] != 0xffffffffu) rk[k] = half16(old[k], dg[k] & 1u);
        }
        if (lane == 0 && dead_run) atomicAdd(&s_wc[w][(B - 1) >> 1], dead_run << 16);   // B - 1 is odd: high half
        __syncthreads();
        // per word (two buckets): exclusive prefix over the waves in place, tile counts kept
        // (halves <= TILE <= 32,768: no carry between them)
        uint32_t tc[kWPer];
#pragma unroll
        for (int q = 0; q < kWPer; q++) {
            const uint32_t j = t + q * TH;
            tc[q] = 0;
            if (j < kW) {
                uint32_t c[NW];
#pragma unroll
                for (int v = 0; v < NW; v++) c[v] = s_wc[v][j];
                uint32_t run = 0;
#pragma unroll
                for (int v = 0; v < NW; v++) {
                    s_wc[v][j] = run;
                    run += c[v];
                }
                tc[q] = run;
            }
        }
        if (STAGED) {
            // the buckets' offsets in the tile: thread t < kW scans word t's two tile counts
            const uint32_t lo = tc[0] & 0xffffu, hi = tc[0] >> 16;
            uint32_t tot;
            const uint32_t ex = block_exclusive_scan_lead<uint32_t, NW>(t < kW ? lo + hi : 0u, s_scr, tot);
            if (t < kW) {
                s_tp[2 * t] = ex;
                s_tp[2 * t + 1] = ex + lo;
            }
        }
        __syncthreads();
        if (STAGED) {
#pragma unroll
            for (int k = 0; k < kIt; k++) {
                const uint32_t el = wbase + k * 64 + lane;
                if (el < tn) {
                    const uint32_t d = dg[k];
                    const uint32_t p = s_tp[d] + half16(s_wc[w][d >> 1], d & 1u) + rk[k];
                    s_stage[p] = make_uint4((uint32_t)it[k], (uint32_t)(it[k] >> 32), pv[k], d);
                }
            }
            __syncthreads();
            // the counters' last read is behind: clear them for the next tile
            for (uint32_t j = t; j < NW * kW; j += TH) (&s_wc[0][0])[j] = 0;
            for (uint32_t q = t; q < tn; q += TH) {
                const uint4 r = s_stage[q];
                const uint32_t d = r.w;
                const uint32_t dst = s_gbase[d] + (q - s_tp[d]);
                if (d == (uint32_t)B - 1u) {
                    out[dst] = ((uint64_t)r.y << 32) | r.x;
                    pay_out[dst] = r.z;
                } else {
                    rec_put<true>(rec, dst, r.x, r.y, r.z);
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < kIt; k++) {
                const uint32_t el = wbase + k * 64 + lane;
                if (el < tn) {
                    const uint32_t d = dg[k];
                    const uint32_t dst = s_gbase[d] + half16(s_wc[w][d >> 1], d & 1u) + rk[k];
                    if (d == (uint32_t)B - 1u) {
                        out[dst] = it[k];
                        pay_out[dst] = pv[k];
                    } else {
                        rec_put<false>(rec, dst, (uint32_t)it[k], (uint32_t)(it[k] >> 32), pv[k]);
                    }
                }
            }
        }
        if (more) {
#pragma unroll
            for (int k = 0; k < kIt; k++) {
                it[k] = nit[k];
                pv[k] = npv[k];
                if (STAGED) bv[k] = nbv[k];
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kWPer; q++) {
            const uint32_t j = t + q * TH;
            if (j < kW) {
                s_gbase[2 * j] += tc[q] & 0xffffu;
                s_gbase[2 * j + 1] += tc[q] >> 16;
            }
        }
        // the next tile's barrier after the ranking atomics (STAGED), or its counter clear and
        // barrier (unstaged), orders these updates before their use
    }
}

// Next frame's splitters from this bucket's part of the sorted live order: splitter j is
// the key at live position floor((j + 1) * live / (B - 1)), j < B - 2.  key_at(q) reads
// the sorted key at bucket-local position q.
// Where splitter j (j < B - 2) is taken in a sorted live order of `live` items: the open
// first and last live buckets get a quarter of an interior bucket's share, so a moving
// camera's drift past the previous frame's nearest and farthest keys (which lands in
// them) has room under the local capacity (config 2 on a 0.25-deg orbit, the first frames
// after the LSD quantiles: the last bucket held 2,058 items, over the 2,048 capacity, at
// an even split).  pos(j) = floor(N(j) live / D), N(j) = (B - 3) + j (4B - 6),
// D = 4 (B - 3)(B - 1): pos(0) = live / (4 (B - 1)), pos(B - 3) = live (1 - 1 / (4 (B - 1))).
template <int B>
__device__ __forceinline__ uint32_t bkt_split_pos(uint32_t j, uint32_t live) {
    constexpr uint64_t D = 4ull * (uint64_t)(B - 3) * (uint64_t)(B - 1);
    return (uint32_t)(((uint64_t)(B - 3) + (uint64_t)j * (uint64_t)(4 * B - 6)) * live / D);
}
// The smallest j with bkt_split_pos(j, live) >= s (live > 0).
template <int B>
__device__ __forceinline__ uint64_t bkt_split_first(uint64_t s, uint32_t live) {
    constexpr uint64_t D = 4ull * (uint64_t)(B - 3) * (uint64_t)(B - 1);
    const uint64_t c = (s * D + live - 1) / live;   // pos(j) >= s  <=>  N(j) >= c
    return c <= (uint64_t)(B - 3) ? 0ull : (c - (uint64_t)(B - 3) + (uint64_t)(4 * B - 7)) / (uint64_t)(4 * B - 6);
}

template <int B, int TH = kBktThreads, typename KeyAt>
__device__ __forceinline__ void bkt_write_splitters(uint32_t start, uint32_t count, uint32_t live,
                                                    uint32_t* __restrict__ s_out, KeyAt key_at) {
    if (live == 0 || count == 0) return;
    // splitters j in [j0, j1) are taken at positions in [start, start + count)
    const uint64_t j0 = bkt_split_first<B>(start, live);
    const uint64_t j1 = min(bkt_split_first<B>((uint64_t)start + count, live), (uint64_t)B - 2u);
    for (uint64_t j = j0 + threadIdx.x; j < j1; j += TH)
        s_out[j] = key_at(bkt_split_pos<B>((uint32_t)j, live) - start);
}

// Row-pass histograms of one chunk of the depth order (k_bin_rows_count's, for the chunk
// of the bucket this workgroup sorted): per tile row the row items and the pairs of its
// rects, as difference arrays in LDS (per wave), then a prefix over the rows.
// hist[row][g] and hist[256 + row][g], rows < tiles_y.
struct RowHist {
    uint32_t* hist;      // nullptr: not fused (the row pass counts for itself)
    int groups;          // the row pass's chunks: the live buckets (B - 1)
    int tiles_y;
};

__device__ __forceinline__ void row_hist_add(uint32_t (*h_items)[256], uint32_t (*h_pairs)[256], uint32_t w,
                                             uint32_t packed) {
    const uint64_t r = unpack_rect(packed);
    if (rect_count(r)) {
        const uint32_t ty0 = (uint32_t)((r >> 32) & 0xffffu), ty1 = (uint32_t)(r >> 48);
        const uint32_t cols = rect_cols(r);
        atomicAdd(&h_items[w][ty0], 1u);
        atomicAdd(&h_pairs[w][ty0], cols);
        if (ty1 < 255u) {
            atomicSub(&h_items[w][ty1 + 1], 1u);
            atomicSub(&h_pairs[w][ty1 + 1], cols);
        }
    }
}

__device__ __forceinline__ void row_hist_write(const RowHist& rh, uint32_t g, uint32_t (*h_items)[256],
                                               uint32_t (*h_pairs)[256], uint32_t* s_scr) {
    const uint32_t t = threadIdx.x;
    __syncthreads();
    const uint32_t di = h_items[0][t] + h_items[1][t] + h_items[2][t] + h_items[3][t];
    const uint32_t dp = h_pairs[0][t] + h_pairs[1][t] + h_pairs[2][t] + h_pairs[3][t];
    uint32_t ti, tp;
    const uint32_t ci = block_exclusive_scan<uint32_t>(di, s_scr, ti) + di;
    const uint32_t cp = block_exclusive_scan<uint32_t>(dp, s_scr, tp) + dp;
    if (t < (uint32_t)rh.tiles_y) {
        rh.hist[t * (uint32_t)rh.groups + g] = ci;
        rh.hist[(256 + t) * (uint32_t)rh.groups + g] = cp;
    }
}

// One workgroup per live bucket (grid B - 1; B with the fused row count, whose last
// workgroup only counts the last bucket's rows).  bstart: the buckets' first positions
// (k_bkt_scatter); s_in: the splitters this frame was bucketed by, which bound the keys of
// every bucket but the first and the last (their key span sets the passes).  cap: buckets
// above it take the global path (kBktCap; smaller only as a test hook).  over_host
// (host-mapped, nullable): items sorted by the global path, for the diagnostics.
template <int B, bool RA, bool R12 = false>
__global__ __launch_bounds__(kBktThreads) void k_bkt_local(uint64_t* __restrict__ items, uint64_t* __restrict__ scratch,
                                                           uint32_t* __restrict__ pay, uint32_t* __restrict__ pay_scratch,
                                                           uint32_t* __restrict__ bstart,
                                                           const uint32_t* __restrict__ s_in,
                                                           uint32_t* __restrict__ s_next, uint32_t cap,
                                                           unsigned int* over_host, RowHist rh,
                                                           const uint4* __restrict__ rec,
                                                           const uint32_t* __restrict__ only = nullptr) {
    GSR_GEOM_PRIO();
    __shared__ uint64_t s_items[kBktTile];
    __shared__ uint32_t s_pay[kBktTile];
    __shared__ uint32_t s_wc[4][256], s_lbase[256], s_gb[256];
    __shared__ uint32_t s_hp[4][256];   // fused row-pass count: pairs (s_wc holds the items)
    __shared__ uint32_t s_scr[4], s_mm[2];
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    auto row_zero = [&]() {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            s_wc[k][t] = 0;
            s_hp[k][t] = 0;
        }
    };
    if (blockIdx.x == (uint32_t)B - 1u) {
        // fused row count only (grid B): the last bucket (key 0xFFFFFFFF, index order, never
        // sorted) is the row pass's last chunk.  It holds culled items only unless the scatter
        // raised bstart[B + 1]; then its rects are counted (every live one binned, as the LSD
        // path and render.cu do), else the chunk is emptied (bstart[B] = its start: the
        // row pass reads nothing there).  Only this workgroup reads bstart[B].
        const uint32_t start = bstart[B - 1], end = bstart[B];
        const bool sat = bstart[B + 1] != 0u;
        row_zero();
        __syncthreads();
        if (sat) {
            for (uint32_t i = start + t; i < end; i += 4u * kBktThreads) {
                uint32_t p[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const uint32_t j = i + (uint32_t)k * kBktThreads;
                    p[k] = j < end ? pay[j] : pack_rect(kDeadRect);
                }
#pragma unroll
                for (int k = 0; k < 4; k++) row_hist_add(s_wc, s_hp, w, p[k]);
            }
        }
        row_hist_write(rh, (uint32_t)B - 1u, s_wc, s_hp, s_scr);
        if (!sat && t == 0) bstart[B] = start;
        return;
    }
    // XCD-contiguous buckets: the fused row count's histogram lines (16 consecutive
    // buckets of a row) merge in one L2 (12.4 -> 11.95 us at config 2,
    // profiles/r05_kt_xcd_hist.txt)
    const uint32_t bkt = (uint32_t)xcd_chunk((int)blockIdx.x, B - 1);
    if (only && only[bkt] == 0u) return;   // big buckets: only those k_bbk_local left to this kernel
    const uint32_t start = bstart[bkt], count = bstart[bkt + 1] - start, live = bstart[B - 1];
    // keys of bucket b lie in [s_in[b - 1], s_in[b]) for 0 < b < B - 2
    const bool bounded = bkt > 0 && bkt < (uint32_t)B - 2u;
    const uint32_t klo = bounded ? s_in[bkt - 1] : 0u, khi = bounded ? s_in[bkt] : 0u;
    if (bkt == 0 && t == 0) {
        s_next[B - 2] = 0xffffffffu;
        if (live == 0)   // no live quantiles (a camera looking away): keep this frame's splitters
            for (uint32_t j = 0; j < (uint32_t)B - 2u; j++) s_next[j] = s_in[j];
    }
    if (count == 0) {   // uniform; an empty bucket is an empty row-pass chunk
        if (rh.hist) {
            row_zero();
            row_hist_write(rh, bkt, s_wc, s_hp, s_scr);
        }
        return;
    }
    uint64_t* const seg = items + start;
    uint32_t* const pseg = pay + start;
    auto rseg = [&](uint32_t q) { return rec_get<R12>(rec, start + q); };   // the bucket's records, index order
    // ---- fast path: the bucket in registers, stable 8-bit passes through LDS.  IT items per
    // thread: 4 for buckets of up to 1,024 (the usual ~n / B: every wave holds a quarter of
    // the bucket), 8 up to the capacity (at 8, buckets under 1,024 left waves 2 and 3 idle
    // and waves 0 and 1 with twice the slots) ----
    auto fast = [&](auto it_c) {
        constexpr int IT = decltype(it_c)::value;
        const uint32_t wbase = w * 64 * IT;
        uint64_t it[IT];
        uint32_t pv[IT];
#pragma unroll
        for (int k = 0; k < IT; k++) {
            const uint32_t el = wbase + k * 64 + lane;
            const uint4 r = el < count ? rseg(el) : make_uint4(~0u, ~0u, 0u, 0u);
            it[k] = ((uint64_t)r.y << 32) | r.x;
            pv[k] = r.z;
        }
        uint32_t kmin = klo, span = khi - klo - 1u;   // bounded: keys in [klo, khi)
        if (!bounded) {   // the open-ended first and last buckets: their own min and max
            uint32_t mn = 0xffffffffu, mx = 0;
#pragma unroll
            for (int k = 0; k < IT; k++)
                if (wbase + k * 64 + lane < count) {
                    mn = min(mn, (uint32_t)(it[k] >> 32));
                    mx = max(mx, (uint32_t)(it[k] >> 32));
                }
            mn = ~wave_max_u32(~mn);
            mx = wave_max_u32(mx);
            if (t < 2) s_mm[t] = t ? 0u : 0xffffffffu;
            __syncthreads();
            if (lane == 0) {
                atomicMin(&s_mm[0], mn);
                atomicMax(&s_mm[1], mx);
            }
            __syncthreads();
            kmin = s_mm[0];
            span = s_mm[1] - kmin;
        }
        const int bits = span ? 32 - __clz((int)span) : 0;
        for (int shift = 0; shift < bits; shift += 8) {   // uniform
            uint32_t dig[IT], pos[IT];
#pragma unroll
            for (int k = 0; k < IT; k++) dig[k] = (((uint32_t)(it[k] >> 32) - kmin) >> shift) & 0xffu;
            (void)bin_rank_tile<IT, 8, RA>(dig, count, pos, s_wc, s_lbase, s_scr);
#pragma unroll
            for (int k = 0; k < IT; k++) {
                const uint32_t el = wbase + k * 64 + lane;
                if (el < count) {
                    s_items[pos[k]] = it[k];
                    s_pay[pos[k]] = pv[k];
                }
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < IT; k++) {
                const uint32_t el = wbase + k * 64 + lane;
                if (el < count) {
                    it[k] = s_items[el];
                    pv[k] = s_pay[el];
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int k = 0; k < IT; k++) {
            const uint32_t el = wbase + k * 64 + lane;
            if (el < count) {
                seg[el] = it[k];
                pseg[el] = pv[k];
                s_items[el] = it[k];
            }
        }
        if (rh.hist) {   // the bucket is the row pass's chunk: its row histograms from the rects
            row_zero();
            __syncthreads();
#pragma unroll
            for (int k = 0; k < IT; k++)
                if (wbase + k * 64 + lane < count) row_hist_add(s_wc, s_hp, w, pv[k]);
            row_hist_write(rh, bkt, s_wc, s_hp, s_scr);
        }
        __syncthreads();
        if (bkt < (uint32_t)B - 1u)
            bkt_write_splitters<B>(start, count, live, s_next,
                                   [&](uint32_t q) { return (uint32_t)(s_items[q] >> 32); });
    };
    // (5 and 6 items per thread for the 1,025-1,536-item buckets of scenes above 4M items:
    // at 8 the items of a 1,220-item bucket sat on waves 0-1 and 2-3 idled)
    if (count <= min(cap, (uint32_t)kBktThreads * 4u)) {
        fast(std::integral_constant<int, 4>{});
        return;
    }
    if (count <= min(cap, (uint32_t)kBktThreads * 5u)) {
        fast(std::integral_constant<int, 5>{});
        return;
    }
    if (count <= min(cap, (uint32_t)kBktThreads * 6u)) {
        fast(std::integral_constant<int, 6>{});
        return;
    }
    if (count <= cap) {
        fast(std::integral_constant<int, 8>{});
        return;
    }
    const uint32_t wbase = w * 64 * kBktItems;
    // ---- over capacity: stable 8-bit passes through global memory, one tile at a time ----
    if (over_host && t == 0) atomicAdd_system(over_host, count);
    for (uint32_t i = t; i < count; i += kBktThreads) {   // the records into the item / rect arrays
        const uint4 r = rseg(i);
        seg[i] = ((uint64_t)r.y << 32) | r.x;
        pseg[i] = r.z;
    }
    __threadfence();
    __syncthreads();
    uint32_t kmin = 0xffffffffu, kmax = 0;
    for (uint32_t i = t; i < count; i += kBktThreads) {
        const uint32_t k = (uint32_t)(seg[i] >> 32);
        kmin = min(kmin, k);
        kmax = max(kmax, k);
    }
    kmin = ~wave_max_u32(~kmin);
    kmax = wave_max_u32(kmax);
    if (t < 2) s_mm[t] = t ? 0u : 0xffffffffu;
    __syncthreads();
    if (lane == 0) {
        atomicMin(&s_mm[0], kmin);
        atomicMax(&s_mm[1], kmax);
    }
    __syncthreads();
    kmin = s_mm[0];
    const uint32_t span = s_mm[1] - kmin;
    const int bits = span ? 32 - __clz((int)span) : 0;
    if (over_host && t == 0 && bits) atomicAdd_system(over_host + 1, count * (uint32_t)((bits + 7) / 8));
    uint64_t* src = seg;
    uint64_t* dst = scratch + start;
    uint32_t* psrc = pseg;
    uint32_t* pdst = pay_scratch + start;
    int passes = 0;
    for (int shift = 0; shift < bits; shift += 8, ++passes) {
        auto digit = [&](uint64_t v) { return (((uint32_t)(v >> 32) - kmin) >> shift) & 0xffu; };
        s_gb[t] = 0;
        __syncthreads();
        for (uint32_t i = t; i < count; i += kBktThreads) atomicAdd(&s_gb[digit(src[i])], 1u);
        __syncthreads();
        {
            const uint32_t c = s_gb[t];
            uint32_t tot;
            const uint32_t ex = block_exclusive_scan<uint32_t>(c, s_scr, tot);
            s_gb[t] = ex;   // every read of s_gb[t] (its own count) is done by this thread
        }
        for (uint32_t tb = 0; tb < count; tb += kBktTile) {
            const uint32_t tn = min(kBktTile, count - tb);
            uint64_t it[kBktItems];
            uint32_t pv[kBktItems], dig[kBktItems], pos[kBktItems];
#pragma unroll
            for (int k = 0; k < kBktItems; k++) {
                const uint32_t el = wbase + k * 64 + lane;
                it[k] = el < tn ? src[tb + el] : ~0ull;
                pv[k] = el < tn ? psrc[tb + el] : 0u;
                dig[k] = digit(it[k]);
            }
            const uint32_t tcount = bin_rank_tile<kBktItems, 8, RA>(dig, tn, pos, s_wc, s_lbase, s_scr);
#pragma unroll
            for (int k = 0; k < kBktItems; k++) {
                const uint32_t el = wbase + k * 64 + lane;
                if (el < tn) {
                    s_items[pos[k]] = it[k];
                    s_pay[pos[k]] = pv[k];
                }
            }
            __syncthreads();
            for (uint32_t q = t; q < tn; q += kBktThreads) {
                const uint64_t v = s_items[q];
                const uint32_t d = digit(v);
                const uint32_t o = s_gb[d] + (q - s_lbase[d]);
                dst[o] = v;
                pdst[o] = s_pay[q];
            }
            __syncthreads();
            s_gb[t] += tcount;
            // bin_rank_tile's first barrier orders this before the next tile's reads
        }
        __threadfence();   // the next pass (other waves of this workgroup) reads what this one wrote
        __syncthreads();
        uint64_t* ts = src;
        src = dst;
        dst = ts;
        uint32_t* tp = psrc;
        psrc = pdst;
        pdst = tp;
    }
    if (passes & 1) {   // the result is in the scratch segment: copy it back
        for (uint32_t i = t; i < count; i += kBktThreads) {
            seg[i] = src[i];
            pseg[i] = psrc[i];
        }
        __threadfence();
        __syncthreads();
    }
    if (rh.hist) {
        row_zero();
        __syncthreads();
        for (uint32_t i = t; i < count; i += kBktThreads) row_hist_add(s_wc, s_hp, w, pseg[i]);
        row_hist_write(rh, bkt, s_wc, s_hp, s_scr);
    }
    if (bkt < (uint32_t)B - 1u)
        bkt_write_splitters<B>(start, count, live, s_next, [&](uint32_t q) { return (uint32_t)(seg[q] >> 32); });
}

// ---- big buckets (scenes above 2M Gaussians: 512 buckets of ~n / 512 items) ----
//
// One 1,024-thread workgroup sorts a bucket of up to 16,384 items in LDS: up to 16 per thread
// (blocked per wave, so a wave's items are consecutive positions; the 16 waves share the
// bucket evenly, ceil(count / 1,024) rows of 64 each, so all of them work), stable 8-bit LSD passes
// over key - lo whose exchange carries one u32 per item, slot (original position, 14 bits) |
// (key - lo) << 14, so keys may span 18 bits above lo (config 3's buckets: 12-13).  After
// the last pass each position knows its slot and key; the index (kept in LDS by slot) and
// the rect (pulled through the exchange buffer by slot) join them and the bucket is written
// out coalesced.  Buckets over the capacity or wider than 18 bits are flagged in `left` and
// sorted by k_bkt_local's paths in a second launch.
constexpr int kBbThreads = 1024;
constexpr int kBbItems = 16;                            // capacity kBbThreads * 16: 16,384

// One workgroup per CU; it reads the staged scatter's 12-B records.
template <bool RA>
__global__ __launch_bounds__(kBbThreads) void k_bbk_local(uint64_t* __restrict__ items, uint32_t* __restrict__ pay,
                                                          const uint32_t* __restrict__ bstart,
                                                          const uint32_t* __restrict__ s_in,
                                                          uint32_t* __restrict__ s_next, uint32_t cap,
                                                          const uint4* __restrict__ rec, uint32_t* __restrict__ left) {
    GSR_GEOM_PRIO();
    constexpr int B = kBigBuckets, TH = kBbThreads;
    constexpr int NW = TH / 64;
    constexpr uint32_t kCap = (uint32_t)TH * kBbItems;
    constexpr int kBbSlot = __builtin_ctz(kCap);        // slot bits of the exchange word
    constexpr int kBbKeyBits = 32 - kBbSlot;            // key bits above lo it carries
    __shared__ uint32_t s_buf[kCap];                    // the exchange, then the rect pull, then the keys
    __shared__ uint32_t s_idx[kCap];                    // the indices by slot
    __shared__ uint32_t s_wc[NW][256];                  // per-wave digit counts, then their wave prefixes
    __shared__ uint32_t s_db[256];                      // the digits' first positions
    __shared__ uint32_t s_scr[NW], s_mm[2];
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    const uint32_t bkt = blockIdx.x;
    const uint32_t start = bstart[bkt], count = bstart[bkt + 1] - start, live = bstart[B - 1];
    const bool bounded = bkt > 0 && bkt < (uint32_t)B - 2u;
    const uint32_t klo = bounded ? s_in[bkt - 1] : 0u, khi = bounded ? s_in[bkt] : 0u;
    if (bkt == 0 && t == 0) {
        s_next[B - 2] = 0xffffffffu;
        if (live == 0)   // no live quantiles (a camera looking away): keep this frame's splitters
            for (uint32_t j = 0; j < (uint32_t)B - 2u; j++) s_next[j] = s_in[j];
    }
    if (count == 0) {
        if (t == 0) left[bkt] = 0u;
        return;
    }
    if (count > min(cap, kCap)) {
        if (t == 0) left[bkt] = 1u;
        return;
    }
    // the waves split the bucket evenly (kk rows of 64 each) so every wave has work
    const uint32_t kk = (count + NW * 64u - 1u) / (NW * 64u), wbase = w * kk * 64u;
    uint32_t x[kBbItems], rct[kBbItems];
    {
        uint32_t key[kBbItems];
#pragma unroll
        for (int k = 0; k < kBbItems; k++) {
            const uint32_t el = wbase + k * 64 + lane;
            const bool in = k < (int)kk && el < count;
            const uint4 r = in ? rec_get<true>(rec, start + el) : make_uint4(0u, 0xffffffffu, 0u, 0u);
            if (in) s_idx[el] = r.x;
            key[k] = r.y;
            rct[k] = r.z;
        }
        uint32_t kmin = klo, span = khi - klo - 1u;
        if (!bounded) {   // the open first and last buckets: their own min and max
            uint32_t mn = 0xffffffffu, mx = 0;
#pragma unroll
            for (int k = 0; k < kBbItems; k++)
                if (k < (int)kk && wbase + k * 64 + lane < count) {
                    mn = min(mn, key[k]);
                    mx = max(mx, key[k]);
                }
            mn = ~wave_max_u32(~mn);
            mx = wave_max_u32(mx);
            if (t < 2) s_mm[t] = t ? 0u : 0xffffffffu;
            __syncthreads();
            if (lane == 0) {
                atomicMin(&s_mm[0], mn);
                atomicMax(&s_mm[1], mx);
            }
            __syncthreads();
            kmin = s_mm[0];
            span = s_mm[1] - kmin;
        }
        if (span >> kBbKeyBits) {   // uniform: wider than the exchange word (k_bkt_local sorts it)
            if (t == 0) left[bkt] = 1u;
            return;
        }
        // the exchange word of every position (before the first pass: position = slot)
#pragma unroll
        for (int k = 0; k < kBbItems; k++) x[k] = (wbase + k * 64 + lane) | ((key[k] - kmin) << kBbSlot);
        __syncthreads();   // every thread has read s_mm before it is rewritten
        if (t == 0) {
            left[bkt] = 0u;
            s_mm[0] = kmin;
            s_mm[1] = span;
        }
    }
    __syncthreads();
    const uint32_t kmin = s_mm[0], span = s_mm[1];
    const int bits = span ? 32 - __clz((int)span) : 0;   // the passes: the bits the keys span
    for (int shift = 0; shift < bits; shift += 8) {   // uniform
        auto digit = [&](int k) { return (x[k] >> (kBbSlot + shift)) & 0xffu; };
        for (uint32_t j = t; j < (uint32_t)NW * 256u; j += TH) (&s_wc[0][0])[j] = 0;
        __syncthreads();
        uint32_t rk[kBbItems];
#pragma unroll
        for (int k = 0; k < kBbItems; k++) {
            rk[k] = 0;
            if (k >= (int)kk) continue;   // uniform
            const uint32_t el = wbase + k * 64 + lane;
            const bool valid = el < count;
            const uint32_t dk = digit(k);
            if (RA) {
                rk[k] = atomicAdd(&s_wc[w][dk], valid ? 1u : 0u);
            } else {
                const uint64_t peers = match_peers<8>(dk, valid, 8);
                rk[k] = 0;
                if (valid) {
                    rk[k] = s_wc[w][dk] + (uint32_t)__popcll(peers & (lane ? (~0ull >> (64 - lane)) : 0ull));
                    if (lane == (uint32_t)(__ffsll((unsigned long long)peers) - 1))
                        atomicAdd(&s_wc[w][dk], (uint32_t)__popcll(peers));
                }
            }
        }
        __syncthreads();
        uint32_t dtot = 0;
        if (t < 256u) {
            uint32_t run = 0;
#pragma unroll
            for (int v = 0; v < NW; v++) {
                const uint32_t c = s_wc[v][t];
                s_wc[v][t] = run;
                run += c;
            }
            dtot = run;
        }
        {
            uint32_t tot;
            const uint32_t ex = block_exclusive_scan<uint32_t, NW>(dtot, s_scr, tot);
            if (t < 256u) s_db[t] = ex;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kBbItems; k++) {
            const uint32_t el = wbase + k * 64 + lane;
            if (k < (int)kk && el < count) {
                const uint32_t dk = digit(k);
                s_buf[s_db[dk] + s_wc[w][dk] + rk[k]] = x[k];
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kBbItems; k++) {
            const uint32_t el = wbase + k * 64 + lane;
            if (k < (int)kk && el < count) x[k] = s_buf[el];
        }
        __syncthreads();
    }
    // rect by slot through the buffer (owners write by slot, positions read), then write out
#pragma unroll
    for (int k = 0; k < kBbItems; k++)
        if (k < (int)kk && wbase + k * 64 + lane < count) s_buf[wbase + k * 64 + lane] = rct[k];
    __syncthreads();
    uint64_t* const seg = items + start;
    uint32_t* const pseg = pay + start;
#pragma unroll
    for (int k = 0; k < kBbItems; k++) {
        const uint32_t el = wbase + k * 64 + lane;
        if (k < (int)kk && el < count) {
            const uint32_t slot = x[k] & (kCap - 1u);
            rct[k] = s_buf[slot];
            seg[el] = ((uint64_t)(kmin + (x[k] >> kBbSlot)) << 32) | s_idx[slot];
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kBbItems; k++) {
        const uint32_t el = wbase + k * 64 + lane;
        if (k < (int)kk && el < count) {
            pseg[el] = rct[k];
            s_buf[el] = kmin + (x[k] >> kBbSlot);   // sorted keys, for the next frame's splitters
        }
    }
    __syncthreads();
    if (bkt < (uint32_t)B - 1u)
        bkt_write_splitters<B, TH>(start, count, live, s_next, [&](uint32_t q) { return s_buf[q]; });
}

// Splitters from a depth order the LSD passes sorted (a context's first frame, or the
// first after the bucket count changed): one workgroup.  live (nullable): the visible
// count of a partitioned sort; else the first key 0xFFFFFFFF is found by two rounds of
// 256 probes and a last scan.
template <int B>
__global__ __launch_bounds__(kBktThreads) void k_bkt_splitters(const uint64_t* __restrict__ items0,
                                                               const uint64_t* __restrict__ items1,
                                                               const uint32_t* __restrict__ dstats, uint32_t n,
                                                               const uint32_t* __restrict__ live_dev,
                                                               uint32_t* __restrict__ s_out) {
    GSR_GEOM_PRIO();
    __shared__ uint32_t s_lo, s_hi;
    const uint64_t* sorted = depth_sorted(items0, items1, dstats);
    const uint32_t t = threadIdx.x;
    uint32_t live;
    if (live_dev) {
        live = min(*live_dev, n);
    } else {
        // the first position whose key is 0xFFFFFFFF (n if none): narrow [lo, hi) by probes
        if (t == 0) {
            s_lo = 0;
            s_hi = n;
        }
        __syncthreads();
        for (int round = 0; round < 3; round++) {
            const uint32_t lo = s_lo, hi = s_hi;
            __syncthreads();
            const uint32_t len = hi - lo;
            if (len <= 1) break;   // uniform
            const uint32_t step = (len + kBktThreads - 1) / kBktThreads;
            const uint32_t p = lo + t * step;
            const bool dead = p < hi && (uint32_t)(sorted[p] >> 32) == 0xffffffffu;
            // the last probe that is live, then the first that is dead, bound the answer
            if (p < hi && !dead) atomicMax(&s_lo, p + 1);
            if (dead) atomicMin(&s_hi, p);
            __syncthreads();
        }
        uint32_t lo = s_lo;
        const uint32_t hi = s_hi;
        __syncthreads();
        // at most a few positions left: each thread checks one
        if (t == 0) s_lo = hi;
        __syncthreads();
        for (uint32_t p = lo + t; p < hi; p += kBktThreads)
            if ((uint32_t)(sorted[p] >> 32) == 0xffffffffu) atomicMin(&s_lo, p);
        __syncthreads();
        live = s_lo;
        (void)lo;
    }
    // thread t takes splitters t * kPer .. + kPer - 1 and makes them non-decreasing with a
    // running max (an order the host's pass budget left incomplete — that frame re-renders
    // — must still give sorted splitters: the bucket search assumes them)
    constexpr int kPer = B / kBktThreads;
    __shared__ uint32_t s_wmax[4];
    uint32_t v[kPer], run = 0;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const uint32_t j = t * kPer + k;
        v[k] = live && j < (uint32_t)B - 2u ? (uint32_t)(sorted[bkt_split_pos<B>(j, live)] >> 32) : 0u;
        v[k] = min(v[k], 0xfffffffeu);
        run = max(run, v[k]);
        v[k] = run;
    }
    // inclusive max over the wave's threads, then over earlier waves
    const uint32_t lane = t & 63u, w = t >> 6;
    const uint32_t x = wave_incl_scan(run, OpMax{});
    if (lane == 63) s_wmax[w] = x;
    uint32_t before = wave_shr1(x);
    __syncthreads();
    for (uint32_t k = 0; k < w; k++) before = max(before, s_wmax[k]);
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const uint32_t j = t * kPer + k;
        if (j < (uint32_t)B - 2u) s_out[j] = max(before, v[k]);
    }
    if (t == 0) s_out[B - 2] = 0xffffffffu;
}

}  // namespace

// ------------------------------------------------------------------ launchers

template <int B>
static void bucket_sort_b(const uint64_t* in, uint64_t* items0, uint64_t* items1, uint32_t n, int groups,
                          const uint32_t* s_in, uint32_t* s_out, uint32_t* hist, uint32_t* totals,
                          const uint32_t* rect, uint32_t* pay0, uint32_t* pay1, bool rank_atomic, uint32_t cap,
                          unsigned int* over_host, hipStream_t s, int row_tiles_y, uint4* rec) {
    // fused row-pass count: the row hist overwrites the bucket hist, which only the scatter reads
    // (grid B with it: the last bucket is the row pass's last chunk, k_bkt_local)
    const RowHist rh{row_tiles_y > 0 ? hist : nullptr, B, row_tiles_y};
    const int local_grid = row_tiles_y > 0 ? B : B - 1;
    uint32_t* bstart = totals + B;   // B + 2 words after the totals
    constexpr int kScTh = B >= 512 ? 512 : kBktThreads;   // k_bkt_scatter's workgroup size
    hipLaunchKernelGGL(k_bkt_count<B>, dim3(groups), dim3(kBktThreads), 0, s, in, n, s_in, groups, hist,
                       static_cast<uint16_t*>(nullptr));
    hipLaunchKernelGGL(k_bkt_scan<B>, dim3(B / 64), dim3(1024), 0, s, hist, groups, totals);
    with_bool(rank_atomic, [&](auto ra) {
        constexpr bool RA = decltype(ra)::value;
        hipLaunchKernelGGL((k_bkt_scatter<B, RA, kScTh, false>), dim3(groups), dim3(kScTh), 0, s, in, items0, n, s_in,
                           groups, hist, static_cast<const uint32_t*>(totals), rect, pay0, bstart, rec,
                           static_cast<const uint16_t*>(nullptr));
        hipLaunchKernelGGL((k_bkt_local<B, RA>), dim3(local_grid), dim3(kBktThreads), 0, s, items0, items1, pay0,
                           pay1, bstart, s_in, s_out, cap, over_host, rh, static_cast<const uint4*>(rec));
    });
}

hipError_t launch_bucket_sort(const uint64_t* in, uint64_t* items0, uint64_t* items1, uint32_t n, int buckets,
                              int groups, const uint32_t* s_in, uint32_t* s_out, uint32_t* hist, uint32_t* totals,
                              const uint32_t* rect, uint32_t* pay0, uint32_t* pay1, bool rank_atomic, uint32_t cap,
                              unsigned int* over_host, hipStream_t s, int row_tiles_y, uint4* rec) {
    if (groups < 1 || groups > kBktMaxGroups || (int64_t)groups * buckets > 256 * (int64_t)kMaxSortGroups || cap < 1 ||
        cap > kBktCap ||
        in == items0 || !rect || !pay0 || !pay1 || !rec)   // in may be items1: the scratch is used after the scatter
        return hipErrorInvalidValue;
    if (n == 0 || row_tiles_y > 256 || (int64_t)512 * buckets > 256 * (int64_t)kMaxSortGroups)
        return n == 0 ? hipSuccess : hipErrorInvalidValue;
    switch (buckets) {
    case 256: bucket_sort_b<256>(in, items0, items1, n, groups, s_in, s_out, hist, totals, rect, pay0, pay1, rank_atomic, cap, over_host, s, row_tiles_y, rec); break;
    case 512: bucket_sort_b<512>(in, items0, items1, n, groups, s_in, s_out, hist, totals, rect, pay0, pay1, rank_atomic, cap, over_host, s, row_tiles_y, rec); break;
    case 1024: bucket_sort_b<1024>(in, items0, items1, n, groups, s_in, s_out, hist, totals, rect, pay0, pay1, rank_atomic, cap, over_host, s, row_tiles_y, rec); break;
    case 2048: bucket_sort_b<2048>(in, items0, items1, n, groups, s_in, s_out, hist, totals, rect, pay0, pay1, rank_atomic, cap, over_host, s, row_tiles_y, rec); break;
    case 4096: bucket_sort_b<4096>(in, items0, items1, n, groups, s_in, s_out, hist, totals, rect, pay0, pay1, rank_atomic, cap, over_host, s, row_tiles_y, rec); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// kBigBuckets buckets, each sorted by one kBbThreads-thread workgroup.  The scatter's tile is
// staged (bucket runs written coalesced), barrier-lean (52.0 -> 50.2 us at config 3 orbit) and
// writes 12-B records (16-B: 51.7 -> 50.5 us); the eight-barrier tile, 16-B records and the
// unstaged scatter measured slower (profiles/r06k_big_buckets_c3_orbit.txt, DESIGN.md
// section 3).
hipError_t launch_bucket_sort_big(const uint64_t* in, uint64_t* items0, uint64_t* items1, uint32_t n, int buckets,
                                  int groups, const uint32_t* s_in, uint32_t* s_out, uint32_t* hist, uint32_t* totals,
                                  const uint32_t* rect, uint32_t* pay0, uint32_t* pay1, bool rank_atomic, uint32_t cap,
                                  unsigned int* over_host, hipStream_t s, uint4* rec) {
    constexpr int B = kBigBuckets;
    if (buckets != B || groups < 1 || groups > kBigBucketGroups ||
        (int64_t)groups * buckets > 256 * (int64_t)kMaxSortGroups || cap < 1 || in == items0 || !rect || !pay0 ||
        !pay1 || !rec)
        return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    uint32_t* bstart = totals + B;          // B + 2 words after the totals
    uint32_t* left = totals + 2 * B + 2;    // per bucket: k_bbk_local left it to k_bkt_local
    const RowHist none{nullptr, B, 0};
    // the count hands each item's bucket to the scatter (u16 in pay1, free until the second
    // launch), which then skips its own splitter search
    uint16_t* bid = reinterpret_cast<uint16_t*>(pay1);
    hipLaunchKernelGGL(k_bkt_count<B>, dim3(groups), dim3(kBktThreads), 0, s, in, n, s_in, groups, hist, bid);
    hipLaunchKernelGGL(k_bkt_scan_g, dim3(B / 16), dim3(1024), 0, s, hist, groups, totals);
    with_bool(rank_atomic, [&](auto ra) {
        constexpr bool RA = decltype(ra)::value;
        hipLaunchKernelGGL((k_bkt_scatter<B, RA, 512, true>), dim3(groups), dim3(512), 0, s, in, items0, n, s_in,
                           groups, hist, static_cast<const uint32_t*>(totals), rect, pay0, bstart, rec,
                           static_cast<const uint16_t*>(bid));
        hipLaunchKernelGGL(k_bbk_local<RA>, dim3(B - 1), dim3(kBbThreads), 0, s, items0, pay0,
                           static_cast<const uint32_t*>(bstart), s_in, s_out, cap, static_cast<const uint4*>(rec), left);
        hipLaunchKernelGGL((k_bkt_local<B, RA, true>), dim3(B - 1), dim3(kBktThreads), 0, s, items0, items1, pay0,
                           pay1, bstart, s_in, s_out, min(cap, kBktCap), over_host, none,
                           static_cast<const uint4*>(rec), static_cast<const uint32_t*>(left));
    });
    return hipGetLastError();
}

hipError_t launch_bkt_splitters(const uint64_t* items0, const uint64_t* items1, const uint32_t* dstats, uint32_t n,
                                const uint32_t* live_dev, int buckets, uint32_t* s_out, hipStream_t s) {
    switch (buckets) {
    case 256: hipLaunchKernelGGL(k_bkt_splitters<256>, dim3(1), dim3(kBktThreads), 0, s, items0, items1, dstats, n, live_dev, s_out); break;
    case 512: hipLaunchKernelGGL(k_bkt_splitters<512>, dim3(1), dim3(kBktThreads), 0, s, items0, items1, dstats, n, live_dev, s_out); break;
    case 1024: hipLaunchKernelGGL(k_bkt_splitters<1024>, dim3(1), dim3(kBktThreads), 0, s, items0, items1, dstats, n, live_dev, s_out); break;
    case 2048: hipLaunchKernelGGL(k_bkt_splitters<2048>, dim3(1), dim3(kBktThreads), 0, s, items0, items1, dstats, n, live_dev, s_out); break;
    case 4096: hipLaunchKernelGGL(k_bkt_splitters<4096>, dim3(1), dim3(kBktThreads), 0, s, items0, items1, dstats, n, live_dev, s_out); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace gsr

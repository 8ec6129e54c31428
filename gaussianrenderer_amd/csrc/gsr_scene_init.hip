// gsr_scene_init.hip — scene initialisation from a point cloud (include/gsr.h "scene
// initialisation"): the exact 3-nearest-neighbour statistic (gsr_points_knn_dist2) and the
// fill that turns points, colours and that statistic into a new scene block
// (gsr_scene_from_points).
//
// The statistic is exact whatever the structure below does: the structure only decides which
// points a lane never looks at, and a point is skipped only behind a box whose float32 lower
// bound, formed by the rule's own expression, is strictly greater than the lane's third best.
//
//   1. k_knn_bounds   bounds of the valid points (ordered-integer atomics in the scratch), the
//                     count of invalid ones
//   2. k_knn_keys     a 63-bit Morton key per point (21 bits per axis over those bounds); an
//                     invalid point's key is all ones, so it sorts behind every valid one
//   3. the sort       the project's stable 8-bit LSD pass (launch_radix_pass) sorts items of
//                     (32 key bits << 32 | index): four passes on the key's low word, the items
//                     re-keyed in place with the high word, four more passes.  Stable, so equal
//                     keys stay in index order and the order is deterministic.
//   4. k_knn_leaves   positions gathered into sorted planes; one wave per leaf of kKnnLeaf
//                     consecutive points forms the leaf's min/max box
//   5. k_knn_boxes    two coarser box levels, kKnnFan children each
//   6. k_knn_search   one lane per point, one wave per leaf, every decision wave-uniform
#include "gsr_device.h"

namespace gsr {

namespace {

static_assert(kKnnLeaf == 64 && kKnnFan == 64, "a leaf and a node's children are one wave64");

// Words of the scratch's head: the bounds as ordered integers, the invalid count.
enum { kHeadLo = 0, kHeadHi = 3, kHeadInvalid = 6, kHeadWords = 64 };

// The scratch: every part 256-B aligned, offsets in bytes.
struct KnnLayout {
    size_t head, items0, items1, hist, totals, high, planes, box0, box1, box2, total;
    uint32_t L, L1, L2;   // leaves, level-1 and level-2 nodes for n points
    int64_t npad;         // L * kKnnLeaf
    int groups;           // workgroups of a sort pass
};

inline size_t align256(size_t b) { return (b + 255u) & ~(size_t)255u; }

KnnLayout knn_layout(int64_t n) {
    KnnLayout a{};
    a.L = (uint32_t)((n + kKnnLeaf - 1) / kKnnLeaf);
    a.L1 = (a.L + kKnnFan - 1) / kKnnFan;
    a.L2 = (a.L1 + kKnnFan - 1) / kKnnFan;
    a.npad = (int64_t)a.L * kKnnLeaf;
    a.groups = (int)std::max<int64_t>(1, std::min<int64_t>((n + kSortTile - 1) / kSortTile, kMaxSortGroups));
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t o = at;
        at += align256(bytes);
        return o;
    };
    a.head = take(kHeadWords * sizeof(uint32_t));
    a.items0 = take(sizeof(uint64_t) * (size_t)n);
    a.items1 = take(sizeof(uint64_t) * (size_t)n);
    a.hist = take(sizeof(uint32_t) * 256u * (size_t)a.groups);
    a.totals = take(sizeof(uint32_t) * 256u);
    a.high = take(sizeof(uint32_t) * (size_t)n);
    a.planes = take(sizeof(float) * 3u * (size_t)a.npad);
    a.box0 = take(sizeof(float) * 6u * (size_t)a.L);
    a.box1 = take(sizeof(float) * 6u * (size_t)a.L1);
    a.box2 = take(sizeof(float) * 6u * (size_t)a.L2);
    a.total = at;
    return a;
}

// A float as an unsigned integer of the same order (-inf lowest), and back.
__device__ __forceinline__ uint32_t ordered_bits(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ordered_float(uint32_t o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

__device__ __forceinline__ bool finite3(float x, float y, float z) {
    return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;   // false for NaN
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o, 64));
    return v;
}
__device__ __forceinline__ uint32_t wave_max_x_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_min_f32(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_max_f32(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

struct PointSource {
    const float* xyz;
    int64_t ps, cs;   // point and component strides, in elements
    uint32_t n;
};

// ------------------------------------------------------------------ bounds

__global__ __launch_bounds__(64) void k_knn_init(uint32_t* __restrict__ head) {
    const uint32_t t = threadIdx.x;
    head[t] = t < kHeadHi ? 0xffffffffu : 0u;
}

// A workgroup takes kKnnBoundsChunk points, item r * 256 + t of the chunk for thread t; its
// seven results leave through one integer atomic each.
__global__ __launch_bounds__(256) void k_knn_bounds(PointSource P, uint32_t* __restrict__ head,
                                                     uint32_t* __restrict__ bad) {
    __shared__ uint32_t s_red[4][7];
    uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u}, inv = 0;
#pragma unroll
    for (int r = 0; r < kKnnBoundsChunk / 256; r++) {
        const uint64_t i = (uint64_t)blockIdx.x * kKnnBoundsChunk + (uint32_t)r * 256u + threadIdx.x;
        if (i >= P.n) continue;
        const float* p = P.xyz + (int64_t)i * P.ps;
        const float v[3] = {p[0], p[P.cs], p[2 * P.cs]};
        if (!finite3(v[0], v[1], v[2])) {
            inv++;
            continue;
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const uint32_t o = ordered_bits(v[c]);
            lo[c] = min(lo[c], o);
            hi[c] = max(hi[c], o);
        }
    }
    const uint32_t w = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        lo[c] = wave_min_u32(lo[c]);
        hi[c] = wave_max_x_u32(hi[c]);
    }
    inv = (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan(inv, OpAdd{}), 63);
    if (lane_id() == 0) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            s_red[w][c] = lo[c];
            s_red[w][3 + c] = hi[c];
        }
        s_red[w][6] = inv;
    }
    __syncthreads();
    const uint32_t t = threadIdx.x;
    if (t < 7) {
        const uint32_t a = s_red[0][t], b = s_red[1][t], c = s_red[2][t], d = s_red[3][t];
        if (t < 3) {
            atomicMin(&head[kHeadLo + t], min(min(a, b), min(c, d)));
        } else if (t < 6) {
            atomicMax(&head[t], max(max(a, b), max(c, d)));
        } else {
            const uint32_t s = a + b + c + d;
            if (s) {
                atomicAdd(&head[kHeadInvalid], s);
                if (bad) atomicAdd(bad, s);
            }
        }
    }
}

// ------------------------------------------------------------------ keys

// Bit k of the low 21 bits of v to bit 3k.
__device__ __forceinline__ uint64_t spread3(uint32_t v) {
    uint64_t x = v & 0x1fffffu;
    x = (x | x << 32) & 0x1f00000000ffffull;
    x = (x | x << 16) & 0x1f0000ff0000ffull;
    x = (x | x << 8) & 0x100f00f00f00f00full;
    x = (x | x << 4) & 0x10c30c30c30c30c3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}

// The cell of v on an axis of [lo, hi]: double arithmetic, so neither the difference nor the
// extent overflows; a zero extent (0 / 0) lands in cell 0.  Only the order comes from it.
__device__ __forceinline__ uint32_t axis_cell(float v, float lo, float hi) {
    const double t = ((double)v - (double)lo) / ((double)hi - (double)lo) * 2097152.0;
    return (uint32_t)fmin(fmax(t, 0.0), 2097151.0);   // fmax(NaN, 0) = 0
}

// items[i] = (the key's low word << 32 | i), high[i] = its high word; an invalid point's
// mean2 is written here (+0), the search never sees it.
__global__ __launch_bounds__(256) void k_knn_keys(PointSource P, const uint32_t* __restrict__ head,
                                                   uint64_t* __restrict__ items, uint32_t* __restrict__ high,
                                                   float* __restrict__ mean2) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= P.n) return;
    const float* p = P.xyz + (int64_t)i * P.ps;
    const float x = p[0], y = p[P.cs], z = p[2 * P.cs];
    if (!finite3(x, y, z)) {
        items[i] = 0xffffffff00000000ull | i;
        high[i] = 0xffffffffu;
        mean2[i] = 0.0f;
        return;
    }
    const uint64_t key = spread3(axis_cell(x, ordered_float(head[kHeadLo + 0]), ordered_float(head[kHeadHi + 0]))) |
                         spread3(axis_cell(y, ordered_float(head[kHeadLo + 1]), ordered_float(head[kHeadHi + 1]))) << 1 |
                         spread3(axis_cell(z, ordered_float(head[kHeadLo + 2]), ordered_float(head[kHeadHi + 2]))) << 2;
    items[i] = (key << 32) | i;
    high[i] = (uint32_t)(key >> 32);   // < 2^31: below every invalid point's
}

__global__ __launch_bounds__(256) void k_knn_rekey(uint64_t* __restrict__ items, const uint32_t* __restrict__ high,
                                                    uint32_t n) {
    const uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    const uint32_t i = (uint32_t)items[p];
    if (i < n) items[p] = ((uint64_t)high[i] << 32) | i;
}

// ------------------------------------------------------------------ leaves and boxes
//
// A level's boxes are six planes of its node count: lo x, y, z, then hi x, y, z.  A node
// without a valid point has lo = +inf, hi = -inf.

// One wave per leaf.  m = the valid points, the first m of the sorted order.
__global__ __launch_bounds__(256) void k_knn_leaves(PointSource P, const uint32_t* __restrict__ head,
                                                     const uint64_t* __restrict__ items, float* __restrict__ planes,
                                                     int64_t npad, float* __restrict__ box, uint32_t L) {
    const uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t leaf = (uint32_t)(p >> 6);
    if (leaf >= L) return;   // the whole wave
    const uint32_t m = P.n - min(head[kHeadInvalid], P.n);
    const bool valid = p < m;
    float v[3] = {0.0f, 0.0f, 0.0f};
    if (valid) {
        const uint32_t i = min((uint32_t)items[p], P.n - 1u);
        const float* q = P.xyz + (int64_t)i * P.ps;
        v[0] = q[0];
        v[1] = q[P.cs];
        v[2] = q[2 * P.cs];
#pragma unroll
        for (int c = 0; c < 3; c++) planes[(int64_t)c * npad + (int64_t)p] = v[c];
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float lo = wave_min_f32(valid ? v[c] : INFINITY);
        const float hi = wave_max_f32(valid ? v[c] : -INFINITY);
        if (lane_id() == 0) {
            box[(size_t)c * L + leaf] = lo;
            box[(size_t)(3 + c) * L + leaf] = hi;
        }
    }
}

// One wave per node of the coarser level: the union of its kKnnFan children.
__global__ __launch_bounds__(256) void k_knn_boxes(const float* __restrict__ in, uint32_t cin,
                                                    float* __restrict__ out, uint32_t cout) {
    const uint32_t node = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (node >= cout) return;
    const uint64_t child = (uint64_t)node * kKnnFan + lane_id();
    const bool ex = child < cin;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float lo = wave_min_f32(ex ? in[(size_t)c * cin + child] : INFINITY);
        const float hi = wave_max_f32(ex ? in[(size_t)(3 + c) * cin + child] : -INFINITY);
        if (lane_id() == 0) {
            out[(size_t)c * cout + node] = lo;
            out[(size_t)(3 + c) * cout + node] = hi;
        }
    }
}

// ------------------------------------------------------------------ the search

// The rule's lower bound between an interval [lo, hi] and a query interval [qlo, qhi] (a point
// when they are equal), per axis; then the rule's own sum.
__device__ __forceinline__ float axis_gap(float lo, float hi, float qlo, float qhi) {
    return fmaxf(fmaxf(lo - qhi, qlo - hi), 0.0f);
}
__device__ __forceinline__ float sum_sq3(float ex, float ey, float ez) { return ((ex * ex) + (ey * ey)) + (ez * ez); }

struct Best3 {
    float b0, b1, b2;   // b0 <= b1 <= b2
    __device__ __forceinline__ void insert(float d) {
        const float n2 = fminf(b2, fmaxf(b1, d));
        const float n1 = fminf(b1, fmaxf(b0, d));
        b0 = fminf(b0, d);
        b1 = n1;
        b2 = n2;
    }
};

struct KnnTree {
    const float* planes;
    int64_t npad;
    const float* box0;
    const float* box1;
    const float* box2;
    uint32_t L, L1, L2;   // the levels' plane strides (node counts for n points)
};

// Lower bound between this lane's child box of a level and the wave's box.
__device__ __forceinline__ float child_bound(const float* __restrict__ box, uint32_t stride, uint64_t child, bool ex,
                                             const float (&wlo)[3], const float (&whi)[3]) {
    if (!ex) return INFINITY;
    float e[3];
#pragma unroll
    for (int c = 0; c < 3; c++)
        e[c] = axis_gap(box[(size_t)c * stride + child], box[(size_t)(3 + c) * stride + child], wlo[c], whi[c]);
    return sum_sq3(e[0], e[1], e[2]);
}

// Every lane takes the `cnt` points of `leaf` (lane j of the wave holds point j); self: the
// wave's own leaf, where lane j skips point j.
__device__ __forceinline__ void scan_leaf(const KnnTree& T, uint32_t leaf, uint32_t m, bool self, float qx, float qy,
                                          float qz, Best3& B) {
    const uint32_t lane = lane_id();
    const uint32_t cnt = (uint32_t)__builtin_amdgcn_readfirstlane((int)min(m - leaf * (uint32_t)kKnnLeaf, (uint32_t)kKnnLeaf));
    const int64_t cp = (int64_t)leaf * kKnnLeaf + lane;
    const bool have = lane < cnt;
    const float cx = have ? T.planes[cp] : 0.0f;
    const float cy = have ? T.planes[T.npad + cp] : 0.0f;
    const float cz = have ? T.planes[2 * T.npad + cp] : 0.0f;
    auto take = [&](uint32_t j) {
        const float xj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cx), (int)j));
        const float yj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cy), (int)j));
        const float zj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cz), (int)j));
        const float dx = xj - qx, dy = yj - qy, dz = zj - qz;
        float d = sum_sq3(dx, dy, dz);
        if (self && j == lane) d = INFINITY;
        B.insert(d);
    };
    if (cnt == (uint32_t)kKnnLeaf) {   // every leaf but the last: a constant trip count unrolls
#pragma unroll 8
        for (uint32_t j = 0; j < (uint32_t)kKnnLeaf; j++) take(j);
    } else {
        for (uint32_t j = 0; j < cnt; j++) take(j);
    }
}

__device__ __forceinline__ float wave_worst(bool valid, float b2) {
    // b2 >= 0 or +inf: its bits order as unsigned integers
    return __uint_as_float(wave_max_u32(valid ? __float_as_uint(b2) : 0u));
}

__global__ __launch_bounds__(256) void k_knn_search(KnnTree T, const uint64_t* __restrict__ items,
                                                     const uint32_t* __restrict__ head, uint32_t n,
                                                     float* __restrict__ mean2) {
    const uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(p >> 6));   // the wave's leaf
    const uint32_t m = n - min(head[kHeadInvalid], n);
    if ((uint64_t)w * kKnnLeaf >= m) return;   // the whole wave
    const uint32_t Lm = (m + kKnnLeaf - 1) / kKnnLeaf;
    const uint32_t L1m = (Lm + kKnnFan - 1) / kKnnFan;
    const uint32_t L2m = (L1m + kKnnFan - 1) / kKnnFan;
    const uint32_t lane = lane_id();
    const bool valid = p < m;
    const float qx = valid ? T.planes[p] : 0.0f;
    const float qy = valid ? T.planes[T.npad + (int64_t)p] : 0.0f;
    const float qz = valid ? T.planes[2 * T.npad + (int64_t)p] : 0.0f;
    Best3 B{INFINITY, INFINITY, INFINITY};

    // the seeds: the wave's own leaf and its neighbours in the order
    scan_leaf(T, w, m, true, qx, qy, qz, B);
    if (w > 0) scan_leaf(T, w - 1, m, false, qx, qy, qz, B);
    if (w + 1 < Lm) scan_leaf(T, w + 1, m, false, qx, qy, qz, B);
    float worst = wave_worst(valid, B.b2);

    float wlo[3], whi[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        wlo[c] = T.box0[(size_t)c * T.L + w];
        whi[c] = T.box0[(size_t)(3 + c) * T.L + w];
    }

    // the walk: a node's children are tested one per lane against the wave's box and the
    // largest third best in the wave; the accepted ones are taken in turn (a bound is tested
    // again when its turn comes: `worst` only shrinks)
    for (uint32_t t2 = 0; t2 < L2m; t2 += kKnnFan) {
        const uint64_t c2 = (uint64_t)t2 + lane;
        const float g2 = child_bound(T.box2, T.L2, c2, c2 < L2m, wlo, whi);
        uint64_t m2 = __ballot(c2 < L2m && !(g2 > worst));
        while (m2) {
            const int k2 = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)m2) - 1);
            m2 &= m2 - 1;
            if (__int_as_float(__builtin_amdgcn_readlane(__float_as_int(g2), k2)) > worst) continue;
            const uint32_t node2 = t2 + (uint32_t)k2;
            const uint64_t c1 = (uint64_t)node2 * kKnnFan + lane;
            const float g1 = child_bound(T.box1, T.L1, c1, c1 < L1m, wlo, whi);
            uint64_t m1 = __ballot(c1 < L1m && !(g1 > worst));
            while (m1) {
                const int k1 = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)m1) - 1);
                m1 &= m1 - 1;
                if (__int_as_float(__builtin_amdgcn_readlane(__float_as_int(g1), k1)) > worst) continue;
                const uint32_t node1 = node2 * (uint32_t)kKnnFan + (uint32_t)k1;
                const uint64_t c0 = (uint64_t)node1 * kKnnFan + lane;
                // the seeds are not taken twice
                const bool ex0 = c0 < Lm && !(c0 + 1 >= w && c0 <= (uint64_t)w + 1);
                const float g0 = child_bound(T.box0, T.L, c0, ex0, wlo, whi);
                uint64_t m0 = __ballot(ex0 && !(g0 > worst));
                while (m0) {
                    const int k0 = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)m0) - 1);
                    m0 &= m0 - 1;
                    if (__int_as_float(__builtin_amdgcn_readlane(__float_as_int(g0), k0)) > worst) continue;
                    const uint32_t leaf = node1 * (uint32_t)kKnnFan + (uint32_t)k0;
                    // the leaf's box against each lane's own point and third best
                    float e[3];
                    const float q[3] = {qx, qy, qz};
#pragma unroll
                    for (int c = 0; c < 3; c++)
                        e[c] = axis_gap(T.box0[(size_t)c * T.L + leaf], T.box0[(size_t)(3 + c) * T.L + leaf], q[c], q[c]);
                    if (!__ballot(valid && !(sum_sq3(e[0], e[1], e[2]) > B.b2))) continue;
                    scan_leaf(T, leaf, m, false, qx, qy, qz, B);
                    worst = wave_worst(valid, B.b2);
                }
            }
        }
    }

    if (!valid) return;
    const uint32_t k = min(3u, m - 1u);
    float r = 0.0f;
    if (k == 3) r = ((B.b0 + B.b1) + B.b2) / 3.0f;
    else if (k == 2) r = (B.b0 + B.b1) / 2.0f;
    else if (k == 1) r = B.b0;
    const uint32_t i = (uint32_t)items[p];
    if (i < n) mean2[i] = r;
}

// ------------------------------------------------------------------ the fill
//
// One thread per Gaussian writes its element of every plane of the new block (each store one
// contiguous run per wave); workgroup 0 also writes the header, as the planar gather does.
struct InitFill {
    PointSource P;
    const float* rgb;   // nullable: 0.5 grey
    int64_t rps, rcs;
    const float* mean2;
    float opacity, min_dist2, scale_mul, scale_max, t_center, t_scale;
    int narrays;
};

__global__ __launch_bounds__(256) void k_scene_init_fill(uint32_t* __restrict__ hdr, float* __restrict__ dst,
                                                          int64_t stride, InitFill F) {
    if (blockIdx.x == 0 && threadIdx.x < GSR_SCENE_HEADER_BYTES / 4) {
        const uint32_t t = threadIdx.x;
        const uint64_t f = t < 6 ? (uint64_t)F.P.n : t < 8 ? (uint64_t)stride : (uint64_t)F.narrays;
        uint32_t wv = 0;
        if (t == 0) wv = GSR_SCENE_MAGIC0;
        else if (t == 1) wv = GSR_SCENE_MAGIC1;
        else if (t == 2) wv = GSR_SCENE_MAGIC2;
        else if (t == 3) wv = GSR_SCENE_MAGIC3;
        else if (t < 10) wv = (t & 1u) ? (uint32_t)(f >> 32) : (uint32_t)f;
        hdr[t] = wv;
    }
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= F.P.n) return;
    auto A = [&](int a) -> float& { return dst[(int64_t)a * stride + (int64_t)i]; };
    // the position's bits, whatever they are
    const uint32_t* p = reinterpret_cast<const uint32_t*>(F.P.xyz) + (int64_t)i * F.P.ps;
    uint32_t* dw = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
    for (int c = 0; c < 3; c++) dw[(int64_t)(GSR_A_X + c) * stride + (int64_t)i] = p[(int64_t)c * F.P.cs];
    A(GSR_A_OPACITY) = F.opacity;
    const float s = fminf(sqrtf(fmaxf(F.mean2[i], F.min_dist2)) * F.scale_mul, F.scale_max);
#pragma unroll
    for (int c = 0; c < 3; c++) A(GSR_A_SCALE0 + c) = s;
    A(GSR_A_ROT0) = 1.0f;
#pragma unroll
    for (int c = 1; c < 4; c++) A(GSR_A_ROT0 + c) = 0.0f;
    const float kShC0 = 0.28209479177387814f;
    const int nsh = (F.narrays == GSR_SCENE_SH3_NARRAYS ? GSR_SCENE_SH3_NARRAYS : GSR_SCENE_NARRAYS) - GSR_A_SH0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float v = F.rgb ? F.rgb[(int64_t)i * F.rps + (int64_t)c * F.rcs] : 0.5f;
        A(GSR_A_SH0 + c) = (v - 0.5f) / kShC0;
    }
    for (int k = 3; k < nsh; k++) A(GSR_A_SH0 + k) = 0.0f;
    if (F.narrays == GSR_SCENE4D_NARRAYS) {
        A(GSR_A_TCENTER) = F.t_center;
        A(GSR_A_TSCALE) = F.t_scale;
        for (int k = 0; k < 9; k++) A(GSR_A_MOTION0 + k) = 0.0f;
    }
}

}  // namespace

// 256 bytes on top of the parts: the launch aligns the caller's pointer up to 256.
int64_t knn_scratch_bytes(int64_t n) { return n <= 0 ? 0 : (int64_t)knn_layout(n).total + 256; }

hipError_t launch_points_knn(const float* xyz, int64_t point_stride, int64_t comp_stride, uint32_t n, float* mean2,
                             uint32_t* bad, void* scratch, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const KnnLayout a = knn_layout(n);
    char* base = static_cast<char*>(scratch);
    base += (256 - reinterpret_cast<uintptr_t>(base) % 256) % 256;
    uint32_t* head = reinterpret_cast<uint32_t*>(base + a.head);
    uint64_t* items0 = reinterpret_cast<uint64_t*>(base + a.items0);
    uint64_t* items1 = reinterpret_cast<uint64_t*>(base + a.items1);
    uint32_t* hist = reinterpret_cast<uint32_t*>(base + a.hist);
    uint32_t* totals = reinterpret_cast<uint32_t*>(base + a.totals);
    uint32_t* high = reinterpret_cast<uint32_t*>(base + a.high);
    float* planes = reinterpret_cast<float*>(base + a.planes);
    float* box0 = reinterpret_cast<float*>(base + a.box0);
    float* box1 = reinterpret_cast<float*>(base + a.box1);
    float* box2 = reinterpret_cast<float*>(base + a.box2);
    const PointSource P{xyz, point_stride, comp_stride, n};

    hipLaunchKernelGGL(k_knn_init, dim3(1), dim3(kHeadWords), 0, s, head);
    hipLaunchKernelGGL(k_knn_bounds, dim3(grid_for(n, kKnnBoundsChunk)), dim3(256), 0, s, P, head, bad);
    hipLaunchKernelGGL(k_knn_keys, dim3(grid_for(n, 256)), dim3(256), 0, s, P, head, items0, high, mean2);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // two stable sorts of four 8-bit passes each end where they began: items0
    for (int half = 0; half < 2; half++) {
        if (half == 1) hipLaunchKernelGGL(k_knn_rekey, dim3(grid_for(n, 256)), dim3(256), 0, s, items0, high, n);
        for (int pass = 0; pass < 4; pass++) {
            e = launch_radix_pass((pass & 1) ? items1 : items0, (pass & 1) ? items0 : items1, nullptr, n, 32 + 8 * pass,
                                  8, a.groups, 16, hist, totals, nullptr, s);
            if (e != hipSuccess) return e;
        }
    }
    hipLaunchKernelGGL(k_knn_leaves, dim3(grid_for(a.npad, 256)), dim3(256), 0, s, P, head, items0, planes, a.npad, box0,
                       a.L);
    hipLaunchKernelGGL(k_knn_boxes, dim3(grid_for(a.L1, 4)), dim3(256), 0, s, box0, a.L, box1, a.L1);
    hipLaunchKernelGGL(k_knn_boxes, dim3(grid_for(a.L2, 4)), dim3(256), 0, s, box1, a.L1, box2, a.L2);
    const KnnTree T{planes, a.npad, box0, box1, box2, a.L, a.L1, a.L2};
    hipLaunchKernelGGL(k_knn_search, dim3(grid_for(a.npad, 256)), dim3(256), 0, s, T, items0, head, n, mean2);
    return hipGetLastError();
}

hipError_t launch_scene_init_fill(void* block, int64_t stride, int narrays, const float* xyz, int64_t point_stride,
                                  int64_t comp_stride, const float* rgb, int64_t rgb_point_stride,
                                  int64_t rgb_comp_stride, uint32_t n, const float* mean2, const gsr_init_config& cfg,
                                  hipStream_t s) {
    const InitFill F{PointSource{xyz, point_stride, comp_stride, n}, rgb, rgb_point_stride, rgb_comp_stride, mean2,
                     cfg.opacity, cfg.min_dist2, cfg.scale_mul, cfg.scale_max, cfg.t_center, cfg.t_scale, narrays};
    hipLaunchKernelGGL(k_scene_init_fill, dim3(std::max(1, grid_for(n, 256))), dim3(256), 0, s,
                       static_cast<uint32_t*>(block),
                       reinterpret_cast<float*>(static_cast<char*>(block) + GSR_SCENE_HEADER_BYTES), stride, F);
    return hipGetLastError();
}

}  // namespace gsr

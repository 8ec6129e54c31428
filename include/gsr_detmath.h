/*
 * gsr_detmath.h — deterministic single-precision elementary functions, compiled
 * IDENTICALLY for the gfx950 kernels (hipcc) and for host code (gcc / clang).
 *
 * Why this exists
 * ---------------
 * The reference renderer (src/core/cuda/render.cu) calls CUDA's libdevice
 * `expf` (render.cu:333, per pixel-splat), `atan2f` (render.cu:719), `cosf`/
 * `sinf` (render.cu:724-725) and `tanf` (render.cu:620).  Their results feed
 * integer quantisers (floorf/ceilf of the AABB, render.cu:748-751) and the
 * alpha / transmittance thresholds of the blend (render.cu:328,335), so a
 * one-ulp difference between the GPU and the CPU oracle can move a pixel by
 * ~1e-3 — ten times the 1e-4 L-inf parity gate.  Both sides therefore use the
 * functions below, which are built only from IEEE-exact primitives
 * (+ - * / with round-to-nearest, fmaf, rintf, fabsf, bit casts) and so give
 * bit-identical results on x86-64 SSE and on CDNA4 VALU, provided the
 * translation unit is compiled with -ffp-contract=off (no implicit FMA) and
 * without fast-math.
 *
 * Accuracy (checked by tests/test_detmath.py against double precision over
 * dense sweeps): expf <= 2 ulp, sin/cos <= 2 ulp on |x| <= pi, atan2f <= 3 ulp,
 * i.e. within the error bounds CUDA documents for the libdevice functions the
 * reference calls (CUDA C Programming Guide, "Mathematical Functions":
 * expf 2 ulp, sinf/cosf 2 ulp, atan2f 3 ulp).  The polynomial coefficients are
 * the published Cephes single-precision minimax sets (S. Moshier), evaluated
 * here with explicit fmaf Horner steps.
 *
 * tanf is NOT restated here: fx/fy (render.cu:620-621) are computed once per
 * frame on the host as a correctly rounded float tan (see gsr_camera_intrinsics
 * in gsr_camera.cpp) and passed to the kernels, so both sides share them.
 */
#ifndef GSR_DETMATH_H
#define GSR_DETMATH_H

#include <stdint.h>
#include <math.h>

#if defined(__HIPCC__)
#define GSR_HD __host__ __device__ __forceinline__
#else
#define GSR_HD static inline
#endif

GSR_HD float gsr_bits_to_float(uint32_t u) {
    union { uint32_t u; float f; } c;
    c.u = u;
    return c.f;
}

GSR_HD uint32_t gsr_float_to_bits(float f) {
    union { uint32_t u; float f; } c;
    c.f = f;
    return c.u;
}

/* float -> int32 with CUDA cvt.rzi.s32.f32 semantics (truncate, saturate,
 * NaN -> 0).  The reference casts with static_cast<int> (render.cu:748-754),
 * which on the GPU saturates; C leaves out-of-range casts undefined, so both
 * sides spell the saturation out. */
GSR_HD int32_t gsr_f2i_sat(float f) {
    if (f != f) return 0;
    if (f >= 2147483648.0f) return 2147483647;
    if (f <= -2147483648.0f) return (-2147483647 - 1);
    return (int32_t)f;
}

/* float -> uint32 with cvt.rzi.u32.f32 semantics: the depth key
 * static_cast<uint32_t>(-Z * 1e6f) (render.cu:850). */
GSR_HD uint32_t gsr_f2u_sat(float f) {
    if (!(f > 0.0f)) return 0u;                 /* NaN, zero, negative */
    if (f >= 4294967296.0f) return 0xffffffffu;
    return (uint32_t)f;
}

/* 2^e as a float for e in [-126, 127] (normal range), built from bits. */
GSR_HD float gsr_pow2i(int e) {
    return gsr_bits_to_float((uint32_t)(e + 127) << 23);
}

/*
 * expf(x): Cody-Waite reduction x = n*ln2 + r, |r| <= ln2/2, then
 * e^r = 1 + r + r^2 * P(r) (Cephes expf coefficients), scaled by 2^n as two
 * exact power-of-two multiplies so the whole finite range (including
 * subnormal results) is covered with IEEE rounding only.
 */
GSR_HD float gsr_expf(float x) {
    /* Branch-free: evaluate on x clamped into [-104, 88.75].  The clamp alone
     * yields the right special results: 2^-150 * e^(-104 + 150 ln2) rounds to
     * +0 for every x <= -104, and 2^128 * e^(88.75 - 128 ln2) overflows to +inf
     * for every x >= 88.75 (ln FLT_MAX = 88.7228); only NaN needs a select. */
    const float xc = fminf(fmaxf(x, -104.0f), 88.75f);   /* NaN -> -104 (replaced below) */
    const float t = xc * 1.44269504088896341f;            /* log2(e) */
    const float n = rintf(t);
    float r = __builtin_fmaf(-n, 0.693359375f, xc);       /* ln2 hi part (exact product) */
    r = __builtin_fmaf(-n, -2.12194440e-4f, r);           /* ln2 lo part */
    float p = 1.9875691500e-4f;
    p = __builtin_fmaf(p, r, 1.3981999507e-3f);
    p = __builtin_fmaf(p, r, 8.3334519073e-3f);
    p = __builtin_fmaf(p, r, 4.1665795894e-2f);
    p = __builtin_fmaf(p, r, 1.6666665459e-1f);
    p = __builtin_fmaf(p, r, 5.0000001201e-1f);
    const float r2 = r * r;
    const float y = __builtin_fmaf(p, r2, r) + 1.0f;
    const int ni = (int)n;                                /* n in [-150, 128] */
#if defined(__HIP_DEVICE_COMPILE__)
    /* v_ldexp_f32: one correctly rounded y * 2^ni — the same value as the two
     * multiplies below (y * 2^e1 is exact and normal, so the second product
     * is the only rounding); gfx950 keeps f32 denormals. */
    const float res = __builtin_amdgcn_ldexpf(y, ni);
#else
    const int e1 = ni / 2;
    const int e2 = ni - e1;
    const float res = (y * gsr_pow2i(e1)) * gsr_pow2i(e2);
#endif
    return (x != x) ? x + x : res;                        /* NaN */
}

/*
 * The blend's expf (render.cu:333, one per pixel-splat pair: the renderer's hottest
 * function).  Same domain handling as gsr_expf (clamp to [-104, 88.75], NaN kept) and
 * the same accuracy class (<= 1.006 ulp against exp over every float, 0.9991 ulp on
 * [-7, 0], monotone non-decreasing on every float: tests/test_detmath.py sweeps it
 * exhaustively), but two instructions cheaper per packed pair on gfx950:
 *   - n = rint(x log2 e) by the 1.5 * 2^23 shifter inside one fma (the rounding of the
 *     exact product, ties to even) instead of a product and two v_rndne_f32;
 *   - a degree-6 minimax e^r = 1 + r + r^2 Q(r) on |r| <= ln2/2 (Q of degree 4, fitted
 *     for relative error 5.5e-9 with float coefficients) instead of Cephes' degree 7.
 * The reference's own expf is CUDA libdevice's, which cannot run here; gsr_expf was
 * the previous stand-in.  Against it this one differs on 0.24 % of all floats, by
 * one ulp; the rendered effect is measured in profiles/r04_blend_exp_parity.txt.
 */
GSR_HD float gsr_blend_expf(float x) {
    const float xc = fminf(fmaxf(x, -104.0f), 88.75f);   /* NaN -> -104 (replaced below) */
    const float t = __builtin_fmaf(xc, 1.44269504088896341f, 12582912.0f);
    const float n = t - 12582912.0f;                      /* rint(xc log2 e), exact */
    float r = __builtin_fmaf(-n, 0.693359375f, xc);
    r = __builtin_fmaf(-n, -2.12194440e-4f, r);
    float q = 0x1.6b42a4p-10f;                            /* 1.38572813e-3 */
    q = __builtin_fmaf(q, r, 0x1.125e6cp-7f);              /* 8.37307237e-3 */
    q = __builtin_fmaf(q, r, 0x1.5557c2p-5f);              /* 4.16678227e-2 */
    q = __builtin_fmaf(q, r, 0x1.555452p-3f);              /* 1.66664734e-1 */
    q = __builtin_fmaf(q, r, 0x1.fffffcp-2f);              /* 4.99999940e-1 */
    const float r2 = r * r;
    const float y = __builtin_fmaf(q, r2, r) + 1.0f;
    const int ni = (int)n;                                /* n in [-150, 128] */
#if defined(__HIP_DEVICE_COMPILE__)
    const float res = __builtin_amdgcn_ldexpf(y, ni);
#else
    const int e1 = ni / 2;
    const int e2 = ni - e1;
    const float res = (y * gsr_pow2i(e1)) * gsr_pow2i(e2);
#endif
    return (x != x) ? x + x : res;
}

/* md2 of renderGaussians (render.cu:331),
 *   dx * (ic0 * dx + ic1 * dy) + dy * (ic2 * dx + ic3 * dy),
 * with the fused multiply-adds the reference's compiler forms: nvcc contracts
 * a * b + c into an FMA by default (--fmad=true) and, like LLVM's combiner, fuses
 * the product that is the sum's FIRST operand.  The blend's accumulation
 * rgb += color * alpha * T (render.cu:337) contracts the same way, to
 * fmaf(color * alpha, T, rgb).  Which product nvcc fuses cannot be observed here
 * (the CUDA path cannot be built); the oracle and the kernels make this one choice
 * together, so they agree bit for bit.  The other choices, measured against this one
 * (profiles/r04_contraction_parity.txt): within 8.7e-5 except the
 * second-product fusion, which moves one config-2 pixel by 1.6e-4. */
GSR_HD float gsr_blend_md2(float dx, float dy, float ic0, float ic1, float ic2, float ic3) {
    return __builtin_fmaf(dx, __builtin_fmaf(ic0, dx, ic1 * dy), dy * __builtin_fmaf(ic2, dx, ic3 * dy));
}

/* Total order of floats as unsigned keys (-inf < ... < -0 < +0 < ... < +inf). */
GSR_HD uint32_t gsr_float_key(float f) {
    const uint32_t b = gsr_float_to_bits(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
GSR_HD float gsr_key_float(uint32_t k) {
    return gsr_bits_to_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

/* The blend's alpha test (render.cu:333-335) as a predicate of the exp argument
 * x = -md2 / 2: is fminf(op * expf(x), 0.99f) >= 1e-3f? */
GSR_HD int gsr_alpha_taken(float op, float x) {
    return !(fminf(op * gsr_blend_expf(x), 0.99f) < 1e-3f);
}

/*
 * Smallest float x with gsr_alpha_taken(op, x): a splat is composited on a pixel
 * (alpha test passed) iff its exp argument -md2/2 >= this value, because
 * gsr_blend_expf is monotone non-decreasing on every float (checked exhaustively on
 * [-104, 88.75], tests/test_gpu_fastexp.py; constant outside) and so is the
 * rounded product op * y for op > 0.  NaN op: alpha = fminf(NaN, 0.99) passes for
 * every x (-inf); op <= 0 never passes (+inf); op = +inf always passes (-inf).
 * For finite op > 0 the answer lies in (-104, 88.75]: gsr_blend_expf(-104) = +0
 * fails and gsr_blend_expf(88.75) = +inf passes.  A few steps from the log estimate find it
 * (the estimate is within a few ulp), with bisection on the float order as the
 * bound.  Host and device give the same value: the estimate only picks where the
 * search starts.
 */
GSR_HD float gsr_alpha_take_min_x(float op) {
    if (op != op) return -INFINITY;
    if (!(op > 0.0f)) return INFINITY;
    if (op == INFINITY) return -INFINITY;
    uint32_t lo = gsr_float_key(-104.0f), hi = gsr_float_key(88.75f);   /* fails / passes */
#if defined(__HIP_DEVICE_COMPILE__)
    float e = __logf(1e-3f / op);
#else
    float e = logf(1e-3f / op);
#endif
    e = fminf(fmaxf(e, -103.0f), 88.0f);
    uint32_t k = gsr_float_key(e);
    for (int s = 0; s < 6 && hi - lo > 1u; s++) {
        if (gsr_alpha_taken(op, gsr_key_float(k))) {
            hi = k;
            k = k - 1u;
        } else {
            lo = k;
            k = k + 1u;
        }
        if (k <= lo || k >= hi) break;
    }
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (gsr_alpha_taken(op, gsr_key_float(mid))) hi = mid;
        else lo = mid;
    }
    return gsr_key_float(hi);
}

/* Polynomial cores on |r| <= pi/4 (Cephes sinf / cosf). */
GSR_HD float gsr_sin_core(float r) {
    const float z = r * r;
    float p = -1.9515295891e-4f;
    p = __builtin_fmaf(p, z, 8.3321608736e-3f);
    p = __builtin_fmaf(p, z, -1.6666654611e-1f);
    return __builtin_fmaf(p * z, r, r);
}

GSR_HD float gsr_cos_core(float r) {
    const float z = r * r;
    float p = 2.443315711809948e-5f;
    p = __builtin_fmaf(p, z, -1.388731625493765e-3f);
    p = __builtin_fmaf(p, z, 4.166664568298827e-2f);
    return __builtin_fmaf(p * z, z, __builtin_fmaf(-0.5f, z, 1.0f));
}

/* Quadrant reduction x = j*pi/2 + r with a three-part pi/2 (Cody-Waite).
 * Accurate for |x| up to ~1e4; the renderer only needs |x| <= pi/2
 * (theta = atan2/2, render.cu:719). Non-finite x gives NaN. */
GSR_HD float gsr_reduce_pio2(float x, int* quadrant) {
    const float j = rintf(x * 0.636619772367581343f);    /* 2/pi */
    float r = __builtin_fmaf(-j, 1.5703125f, x);
    r = __builtin_fmaf(-j, 4.837512969970703125e-4f, r);
    r = __builtin_fmaf(-j, 7.54978995489188216e-8f, r);
    *quadrant = ((int)j) & 3;
    return r;
}

GSR_HD float gsr_sinf(float x) {
    if (!(fabsf(x) < 16384.0f)) return (x - x) / (x - x) ;  /* NaN for inf/NaN/huge */
    int q;
    const float r = gsr_reduce_pio2(x, &q);
    const float s = gsr_sin_core(r);
    const float c = gsr_cos_core(r);
    return (q == 0) ? s : (q == 1) ? c : (q == 2) ? -s : -c;
}

GSR_HD float gsr_cosf(float x) {
    if (!(fabsf(x) < 16384.0f)) return (x - x) / (x - x);
    int q;
    const float r = gsr_reduce_pio2(x, &q);
    const float s = gsr_sin_core(r);
    const float c = gsr_cos_core(r);
    return (q == 0) ? c : (q == 1) ? -s : (q == 2) ? -c : s;
}

/* atan on t >= 0 (Cephes atanf range reduction + minimax polynomial). */
GSR_HD float gsr_atan_pos(float t) {
    float base = 0.0f, base_lo = 0.0f;        /* base = hi + lo (two-part pi/2, pi/4) */
    float u = t;
    if (t > 2.414213562373095f) {             /* tan(3pi/8) */
        base = 1.57079632679489662f;
        base_lo = -4.37113900018624283e-8f;
        u = -1.0f / t;
    } else if (t > 0.4142135623730950f) {     /* tan(pi/8) */
        base = 0.785398163397448310f;
        base_lo = -2.18556950009312141e-8f;
        u = (t - 1.0f) / (t + 1.0f);
    }
    const float z = u * u;
    float p = 8.05374449538e-2f;
    p = __builtin_fmaf(p, z, -1.38776856032e-1f);
    p = __builtin_fmaf(p, z, 1.99777106478e-1f);
    p = __builtin_fmaf(p, z, -3.33329491539e-1f);
    return base + (__builtin_fmaf(p * z, u, u) + base_lo);
}

/* atan2f(y, x) with the C99 Annex F special cases. */
GSR_HD float gsr_atan2f(float y, float x) {
    const float PI = 3.14159265358979323846f;
    const float PI_2 = 1.57079632679489662f;
    const float PI_4 = 0.785398163397448310f;
    const float PI_LO = -8.74227800037248566e-8f;               /* pi - (float)pi */
    if (x != x || y != y) return x + y;                        /* NaN */
    const int ysign = (gsr_float_to_bits(y) >> 31) != 0;
    const int xsign = (gsr_float_to_bits(x) >> 31) != 0;
    const float ay = fabsf(y);
    const float ax = fabsf(x);
    float res;
    if (ay == 0.0f) {
        res = xsign ? PI : 0.0f;                               /* atan2(+-0, x) */
    } else if (ax == 0.0f) {
        res = PI_2;
    } else if (ax == __builtin_inff() && ay == __builtin_inff()) {
        res = xsign ? 3.0f * PI_4 : PI_4;
    } else if (ax == __builtin_inff()) {
        res = xsign ? PI : 0.0f;
    } else if (ay == __builtin_inff()) {
        res = PI_2;
    } else {
        const float a = gsr_atan_pos(ay / ax);
        res = xsign ? ((PI - a) + PI_LO) : a;
    }
    return ysign ? -res : res;
}

/*
 * logf(x) for positive NORMAL floats (the densification sampler's u in (0, 1]; zero,
 * subnormal, negative and non-finite x are not handled).  Cephes logf: x = m 2^e with m in
 * [sqrt(1/2), sqrt(2)) taken from the bits, r = m - 1 (exact), then
 *   log m = r - r^2/2 + r^3 P(r),   log x = log m + e ln2 (ln2 in two parts),
 * in plain float multiplies and adds only — no fma, no libm — so the host and the device
 * round identically.  <= 2 ulp against double precision over every u = k 2^-24, k = 1 ..
 * 2^24 (tests/test_densify_ref.py sweeps them all).
 */
GSR_HD float gsr_logf(float x) {
    const uint32_t b = gsr_float_to_bits(x);
    int e = (int)(b >> 23) - 126;
    float m = gsr_bits_to_float((b & 0x007fffffu) | 0x3f000000u);   /* [0.5, 1) */
    if (m < 0.707106781186547524f) {
        e -= 1;
        m = (m + m) - 1.0f;
    } else {
        m = m - 1.0f;
    }
    const float z = m * m;
    float p = 7.0376836292e-2f;
    p = (p * m) + -1.1514610310e-1f;
    p = (p * m) + 1.1676998740e-1f;
    p = (p * m) + -1.2420140846e-1f;
    p = (p * m) + 1.4249322787e-1f;
    p = (p * m) + -1.6668057665e-1f;
    p = (p * m) + 2.0000714765e-1f;
    p = (p * m) + -2.4999993993e-1f;
    p = (p * m) + 3.3333331174e-1f;
    const float fe = (float)e;
    float y = m * (z * p);
    y = y + (-2.12194440e-4f * fe);
    y = y + (-0.5f * z);
    return (m + y) + (0.693359375f * fe);
}

/*
 * The raw (pre-activation) values a 3DGS .ply stores, from the activated values a scene block
 * holds: the inverses of the loader's exp and sigmoid (gsr_ply.cpp store()), for the PLY writers
 * (gsr_ply_write_host on the host, k_scene_pack on the device).  gsr_logf and plain float
 * operations only, one rounding each, so both writers produce the same bits.
 *
 * gsr_raw_log(s): NaN or s < 0 -> the quiet NaN 0x7fc00000; +-0 -> -inf; +inf -> +inf; a
 * subnormal s is scaled by 2^24 (exact) into the normal range and 24 ln 2 taken off again.
 * Measured against double precision, one value per mantissa step of 2^-12 in every binade
 * from the smallest subnormal to FLT_MAX (tests/test_ply_write.py): <= 0.722 ulp over the
 * normal floats (gsr_logf's <= 2 ulp was only ever swept over (0, 1]), <= 1.006 ulp over the
 * subnormal ones, which pay the subtraction's rounding too.  The test asserts 2 ulp.
 *
 * gsr_raw_logit(o) = log(o) - log(1 - o): NaN or o outside [0, 1] -> the quiet NaN; +-0 ->
 * -inf; 1 -> +inf; exactly 0 at 0.5 (1 - 0.5 is exact and both logs are the same value).
 * Over every o = k 2^-24, k = 1 .. 2^24 - 1 (1 - o is then exact), the bound is ABSOLUTE: the
 * two logs' errors (2 ulp of each asserted) plus half an ulp of the result.  Measured: 0.453 of
 * that bound, 1.373 ulp of the larger log, 9.6e-7 at most (at the ends, where the result is
 * +-16.6); near 0.5 the result is small against its terms and an error of a few 1e-8 is many
 * ulp of the result.
 */
GSR_HD float gsr_raw_log(float s) {
    if (s != s || s < 0.0f) return gsr_bits_to_float(0x7fc00000u);
    if (s == 0.0f) return -INFINITY;
    if (s == INFINITY) return INFINITY;
    if (s < 1.17549435e-38f) return gsr_logf(s * 16777216.0f) - 16.635532f;   /* 24 ln 2 */
    return gsr_logf(s);
}

GSR_HD float gsr_raw_logit(float o) {
    if (o != o || o < 0.0f || o > 1.0f) return gsr_bits_to_float(0x7fc00000u);
    if (o == 0.0f) return -INFINITY;
    if (o == 1.0f) return INFINITY;
    return gsr_raw_log(o) - gsr_raw_log(1.0f - o);
}

/*
 * Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3",
 * SC11; the Random123 generator): ten rounds of two 32 x 32 -> 64 multiplies on a 128-bit
 * counter under a 64-bit key bumped by the Weyl constants between rounds.  The published
 * known-answer vectors are pinned in tests/test_densify_ref.py.
 */
GSR_HD void gsr_philox4x32_10(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4]) {
    uint32_t c0 = counter[0], c1 = counter[1], c2 = counter[2], c3 = counter[3];
    uint32_t k0 = key[0], k1 = key[1];
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

/*
 * The three standard normals of split child `child` of source Gaussian `index`
 * (gsr_scene_densify, include/gsr.h): Philox under key = (seed low word, seed high word) at
 * counter (index, child, 0, 0) gives x0..x3; with u(x) = ((x >> 8) + 1) 2^-24 in (0, 1] and
 * v(x) = (x >> 8) 2^-24 in [0, 1), Box-Muller:
 *   r1 = sqrtf(-2 gsr_logf(u(x0))), a1 = 6.2831855f v(x1): z0 = r1 gsr_cosf(a1), z1 = r1 gsr_sinf(a1)
 *   z2 = sqrtf(-2 gsr_logf(u(x2))) gsr_cosf(6.2831855f v(x3))
 * A sample depends on (seed, index, child) alone; |z| <= sqrt(48 ln 2) = 5.77.
 */
GSR_HD void gsr_densify_normal3(uint64_t seed, uint32_t index, uint32_t child, float z[3]) {
    const uint32_t counter[4] = {index, child, 0u, 0u};
    const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    uint32_t x[4];
    gsr_philox4x32_10(counter, key, x);
    const float s = 5.9604644775390625e-8f;   /* 2^-24 */
    const float r1 = sqrtf(-2.0f * gsr_logf((float)((x[0] >> 8) + 1u) * s));
    const float a1 = 6.2831855f * ((float)(x[1] >> 8) * s);
    const float r2 = sqrtf(-2.0f * gsr_logf((float)((x[2] >> 8) + 1u) * s));
    const float a2 = 6.2831855f * ((float)(x[3] >> 8) * s);
    z[0] = r1 * gsr_cosf(a1);
    z[1] = r1 * gsr_sinf(a1);
    z[2] = r2 * gsr_cosf(a2);
}

#endif /* GSR_DETMATH_H */

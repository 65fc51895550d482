// The arithmetic of a face under a 2 x 3 affine map that gcfr_fullres_affine.hip (one face per photograph) and
// gcfr_fullres_group_affine.hip (every tilted face of a photograph in one launch) share, so that it has ONE text: the fixed point
// (kAffineShift, kAffineOne), the maps of a launch and of a face (AffineArgs, AffineMap), one axis of the carrier (affine_tap), the
// carrier of one pixel (AffineCarrier), the inside test (affine_inside), and on the host the rules of a map (affine_log2k) and a
// launch's argument block (affine_args).  gcfr_fullres_affine.hip's header comment and include/gcfr.h state the formulas.
#pragma once

#include "gcfr_device.hpp"
#include "gcfr_fullres.hpp"

namespace gcfr {

constexpr int kAffineShift = 14;                                  // ONE = 2^14
constexpr int64_t kAffineOne = (int64_t)1 << kAffineShift;

// the maps of one launch, by value in its argument block: m[f] = (M00, M01, M02, M10, M11, M12) of face f
struct AffineArgs {
    int64_t m[kBoxFaces][6];
    int32_t y_lo[kBoxFaces], y_hi[kBoxFaces];     // composite: photograph rows outside [y_lo, y_hi) hold no pixel of the face
    int32_t log2k[kBoxFaces];                     // log2 K(M)
};

// one face's map on the device, with what follows from K
struct AffineMap {
    int64_t m00, m01, m02, m10, m11, m12;
    uint32_t lk;                                  // log2 K
    __device__ AffineMap(const AffineArgs &a, uint32_t f)
        : m00(a.m[f][0]), m01(a.m[f][1]), m02(a.m[f][2]), m10(a.m[f][3]), m11(a.m[f][4]), m12(a.m[f][5]), lk((uint32_t)a.log2k[f]) {}
    __device__ uint32_t K() const { return 1u << lk; }
    __device__ uint32_t shift() const { return (uint32_t)kAffineShift + 1u + lk; }              // log2 den
    // P of sub-sample (0, 0) of destination pixel (x, y)
    __device__ void origin(uint32_t x, uint32_t y, int64_t &P0, int64_t &P1) const
    {
        const int64_t k = (int64_t)1 << lk;
        const int64_t ex = 2 * k * (int64_t)x + 1, ey = 2 * k * (int64_t)y + 1;
        P0 = m00 * ex + m01 * ey + k * (2 * m02 - kAffineOne);
        P1 = m10 * ex + m11 * ey + k * (2 * m12 - kAffineOne);
    }
};

// one axis of the carrier: the two taps, clamped into [0, n), and the weight of the second
__device__ inline void affine_tap(int64_t P, uint32_t shift, uint32_t n, uint32_t &i0, uint32_t &i1, float &t)
{
    const uint64_t U = P > 0 ? (uint64_t)P : 0u;
    const uint64_t q = U >> shift;
    const uint32_t fu = (uint32_t)(U & (((uint64_t)1 << shift) - 1u));
    i0 = q < (uint64_t)(n - 1u) ? (uint32_t)q : n - 1u;
    i1 = i0 + 1u < n ? i0 + 1u : n - 1u;
    t = (float)fu * __builtin_bit_cast(float, (127u - shift) << 23);               // fu / den: fu < 2^18 and den = 2^shift, exact
}

// The carrier of one pixel, beside gcfr_fullres.hpp's Bilinear4: the carried value of the plane whose value at network pixel t is
// value_at(t).  K = 1: the taps are formed once (t00 .. ty).  K > 1: they are recomputed per sub-sample from P of sub-sample (0, 0).
struct AffineCarrier {
    uint32_t lk, shift, h, w;
    int64_t P0, P1, s00, s01, s10, s11;           // P of sub-sample (0, 0); a step of one sub-sample in a, in b (uniform)
    uint32_t t00, t01, t10, t11;
    float tx, ty;
    __device__ AffineCarrier() {}
    __device__ AffineCarrier(const AffineMap &M, int64_t P0_, int64_t P1_, uint32_t h_, uint32_t w_)
        : lk(M.lk), shift(M.shift()), h(h_), w(w_), P0(P0_), P1(P1_), s00(2 * M.m00), s01(2 * M.m01), s10(2 * M.m10), s11(2 * M.m11),
          t00(0u), t01(0u), t10(0u), t11(0u), tx(0.0f), ty(0.0f)
    {
        if (lk == 0u)
            taps(P0, P1, t00, t01, t10, t11, tx, ty);
    }
    __device__ void taps(int64_t p0, int64_t p1, uint32_t &a00, uint32_t &a01, uint32_t &a10, uint32_t &a11, float &fx, float &fy) const
    {
        uint32_t j0, j1, i0, i1;
        affine_tap(p0, shift, w, j0, j1, fx);
        affine_tap(p1, shift, h, i0, i1, fy);
        a00 = i0 * w + j0, a01 = i0 * w + j1, a10 = i1 * w + j0, a11 = i1 * w + j1;
    }
    template <class V>
    __device__ float operator()(V value_at) const
    {
        if (lk == 0u)
            return bilerp(value_at(t00), value_at(t01), value_at(t10), value_at(t11), tx, ty);
        const uint32_t K = 1u << lk;
        double acc = 0.0;
        int64_t r0 = P0, r1 = P1;
        for (uint32_t b = 0; b < K; ++b, r0 += s01, r1 += s11) {
            int64_t p0 = r0, p1 = r1;
            for (uint32_t a = 0; a < K; ++a, p0 += s00, p1 += s10) {
                uint32_t a00, a01, a10, a11;
                float fx, fy;
                taps(p0, p1, a00, a01, a10, a11, fx, fy);
                acc = acc + (double)bilerp(value_at(a00), value_at(a01), value_at(a10), value_at(a11), fx, fy);
            }
        }
        // acc / (double)(K K) as the product with 2^(-2 lk): the same bits (a power of two scales exactly), without the division
        return (float)(acc * __builtin_bit_cast(double, (uint64_t)(1023u - 2u * lk) << 52));
    }
};

// the inside test of one pixel from c = (c0, c1): its centre lands in the network square
__device__ inline bool affine_inside(int64_t c0, int64_t c1, uint64_t lim0, uint64_t lim1)
{
    return (uint64_t)c0 < lim0 && (uint64_t)c1 < lim1;                             // (a negative c is a huge unsigned one)
}

// The rules of include/gcfr.h for one map: det > 0, no column longer than 8, the translations within 2^40.  -> log2 K(M), or -1
inline int affine_log2k(const int64_t *m)
{
    const int64_t lim = (int64_t)8 * kAffineOne;
    if (m[0] < -lim || m[0] > lim || m[1] < -lim || m[1] > lim || m[3] < -lim || m[3] > lim || m[4] < -lim || m[4] > lim)
        return -1;
    if (m[2] < -((int64_t)1 << 40) || m[2] > ((int64_t)1 << 40) || m[5] < -((int64_t)1 << 40) || m[5] > ((int64_t)1 << 40))
        return -1;
    if (m[0] * m[4] - m[1] * m[3] <= 0)
        return -1;
    const int64_t a = m[0] * m[0] + m[3] * m[3], c = m[1] * m[1] + m[4] * m[4], n2 = a > c ? a : c;
    for (int lk = 0; lk < 4; ++lk)
        if ((kAffineOne * kAffineOne) << (2 * lk) >= n2)
            return lk;
    return -1;
}

// n maps -> a launch's argument block; false where a map is refused.  With `rows` (the composite: m = I) the photograph rows the
// network square [0, w] x [0, h] can reach, a superset: row Y of a corner (u, v) solves I (X, Y, 1) = ONE (u, v), exactly.
inline bool affine_args(const int64_t *maps, int32_t n, bool rows, int32_t Hp, int32_t h, int32_t w, AffineArgs &a)
{
    a = {};
    for (int32_t f = 0; f < n; ++f) {
        const int64_t *m = maps + 6 * f;
        const int lk = affine_log2k(m);
        if (lk < 0)
            return false;
        for (int i = 0; i < 6; ++i)
            a.m[f][i] = m[i];
        a.log2k[f] = lk;
        a.y_lo[f] = 0, a.y_hi[f] = Hp;
        if (!rows)
            continue;
        const __int128 det = (__int128)m[0] * m[4] - (__int128)m[1] * m[3];
        __int128 lo = 0, hi = 0;
        for (int corner = 0; corner < 4; ++corner) {
            const __int128 ru = (__int128)kAffineOne * (corner & 1 ? w : 0) - m[2], rv = (__int128)kAffineOne * (corner & 2 ? h : 0) - m[5];
            const __int128 num = (__int128)m[0] * rv - (__int128)m[3] * ru;           // Y = num / det
            __int128 fl = num / det;
            if (num % det != 0 && num < 0)
                --fl;                                                              // floor(Y); ceil(Y) <= floor(Y) + 1
            lo = corner == 0 || fl < lo ? fl : lo;
            hi = corner == 0 || fl > hi ? fl : hi;
        }
        // a pixel's centre y + 1/2 lies in [min Y, max Y]: y >= floor(min Y) - 1 and y < floor(max Y) + 2
        lo -= 1, hi += 2;
        a.y_lo[f] = (int32_t)(lo < 0 ? 0 : lo > Hp ? Hp : lo);
        a.y_hi[f] = (int32_t)(hi < 0 ? 0 : hi > Hp ? Hp : hi);
    }
    return true;
}

}  // namespace gcfr

// The arithmetic of a face box of ANY size that gcfr_fullres_anybox.hip (one box per photograph) and gcfr_fullres_group.hip (every
// face of a photograph in one launch) share, so that it has ONE text: the carrying operator of one axis and of one pixel
// (CarryAxis, carry_axis, carry_1d, AnyCarrier) and one axis of the ingest (IngestAxis, ingest_axis, ingest_tap).
// gcfr_fullres_anybox.hip's header comment and include/gcfr.h state the formulas.
#pragma once

#include "gcfr_device.hpp"
#include "gcfr_fullres.hpp"

namespace gcfr {

// One axis of the carrying operator at box-relative index y of a box axis of nb over a network axis of n (2 nb n < 2^31).
// lerp (nb >= n): the taps i0, i1 and the weight t of i1.  area (nb < n): the first and the last tap i0 .. i1 and lo = y n, the
// start of y's footprint in units of 1 / nb of a network pixel.
struct CarryAxis {
    uint32_t i0, i1, lo;
    float t;
};

__device__ inline CarryAxis carry_axis(bool area, uint32_t y, uint32_t n, uint32_t nb)
{
    CarryAxis a;
    if (area) {
        a.lo = y * n;
        a.i0 = a.lo / nb;
        a.i1 = (a.lo + n + nb - 1u) / nb - 1u;                                     // (<= n - 1: y <= nb - 1)
        a.t = 0.0f;
    } else {
        const uint32_t c = (2u * y + 1u) * n;
        const uint32_t N = c > nb ? c - nb : 0u;
        const uint32_t den = 2u * nb;
        a.i0 = N / den;                                                            // (<= n - 1)
        const uint32_t rem = N - a.i0 * den;
        a.t = (float)((double)rem / (double)den);
        a.i1 = a.i0 + 1u < n ? a.i0 + 1u : n - 1u;
        a.lo = 0u;
    }
    return a;
}

// the operator along one axis: `at(i)` is the value at network index i of that axis
template <class V>
__device__ inline float carry_1d(bool area, const CarryAxis &a, uint32_t n, uint32_t nb, V at)
{
    if (!area) {
        const float a0 = at(a.i0), a1 = at(a.i1);
        return a0 + a.t * (a1 - a0);
    }
    const uint32_t hi = a.lo + n;
    double acc = 0.0;
    for (uint32_t i = a.i0; i <= a.i1; ++i) {
        const uint32_t wt = min((i + 1u) * nb, hi) - max(i * nb, a.lo);
        acc = acc + (double)wt * (double)at(i);
    }
    return (float)(acc / (double)n);
}

// The carrier of one pixel, beside gcfr_fullres.hpp's Bilinear4: the carried value of the plane whose value at network pixel t is
// value_at(t).  ay / ax: is the row / column axis minified (uniform over a workgroup).
struct AnyCarrier {
    bool ay, ax;
    uint32_t h, w, bh, bw;
    CarryAxis Y, X;
    template <class V>
    __device__ float operator()(V value_at) const
    {
        if (!ay && !ax)
            return bilerp(value_at(Y.i0 * w + X.i0), value_at(Y.i0 * w + X.i1), value_at(Y.i1 * w + X.i0), value_at(Y.i1 * w + X.i1),
                          X.t, Y.t);
        return carry_1d(ay, Y, h, bh, [&](uint32_t r) {
            const uint32_t ro = r * w;
            return carry_1d(ax, X, w, bw, [&](uint32_t c) { return value_at(ro + c); });
        });
    }
};

// One axis of the ingest at network index i: slot s of `count` slots is photograph index `first + s` (area) or the tap i0 / i1
// (magnify), with its integer weight.
struct IngestAxis {
    uint32_t first, count, a, b;                   // area: a, b = the cell [i nb, (i+1) nb); magnify: a = i1, b = rem
};

__device__ inline IngestAxis ingest_axis(bool mag, uint32_t i, uint32_t n, uint32_t nb)
{
    IngestAxis x;
    if (mag) {
        const uint32_t c = (2u * i + 1u) * nb;
        const uint32_t N = c > n ? c - n : 0u;
        x.first = N / (2u * n);                                                    // (<= nb - 1)
        x.b = N - x.first * 2u * n;
        x.a = x.first + 1u < nb ? x.first + 1u : nb - 1u;
        x.count = 2u;
    } else {
        x.a = i * nb, x.b = x.a + nb;
        x.first = x.a / n;
        x.count = (x.b + n - 1u) / n - x.first;
    }
    return x;
}

__device__ inline uint32_t ingest_tap(bool mag, const IngestAxis &x, uint32_t s, uint32_t n, uint32_t &weight)
{
    if (mag) {
        weight = s ? x.b : 2u * n - x.b;
        return s ? x.a : x.first;
    }
    const uint32_t y = x.first + s;
    weight = min((y + 1u) * n, x.b) - max(y * n, x.a);
    return y;
}

}  // namespace gcfr

// gcfr::bilinear_weights (two v_fract_f64 per axis) against the reference's floor / ceil / two subtractions, on the device, bit
// for bit (tests/test_gpu_fract_weights.py; the argument: tests/test_fract_weights_host.py).
#include "../../geomconsistentfr_amd/csrc/gcfr_device.hpp"

#include <cstdio>

typedef unsigned long long u64;

enum { kOutside = 0, kInside = 1, kInsideSeen = 2, kTotal = 3, kFirstBad = 4, kSlots = 5 };

__device__ inline double from_bits(u64 b) { return __builtin_bit_cast(double, b); }
__device__ inline u64 to_bits(double d) { return __builtin_bit_cast(u64, d); }
__device__ inline u64 mix(u64 x)  // splitmix64
{
    x += 0x9e3779b97f4a7c15ull;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

// the parent's form (csrc/gcfr_march.hpp: ray_sample, T8:492-494)
__device__ inline void parent_weights(double u, double &w0, double &w1)
{
    w0 = __builtin_ceil(u) - u;
    w1 = u - __builtin_floor(u);
}

struct Tally {
    u64 outside = 0, inside = 0, inside_seen = 0, total = 0, first_bad = ~0ull;
    __device__ void see(double u)
    {
        double a0, a1, b0, b1;
        parent_weights(u, a0, a1);
        gcfr::bilinear_weights(u, b0, b1);
        const bool differ = to_bits(a0) != to_bits(b0) || to_bits(a1) != to_bits(b1);
        const double m = __builtin_fabs(u);
        const bool window = m > 0.0 && m <= 0x1p-54;  // where rn(1 - |u|) = 1.0 (2^-54 itself: the tie goes to 1.0)
        ++total;
        inside_seen += window ? 1 : 0;
        if (differ && window)
            ++inside;
        if (differ && !window) {
            ++outside;
            first_bad = first_bad < to_bits(u) ? first_bad : to_bits(u);
        }
    }
    __device__ void flush(u64 *out) const
    {
        if (outside)
            atomicAdd(out + kOutside, outside);
        if (inside)
            atomicAdd(out + kInside, inside);
        if (inside_seen)
            atomicAdd(out + kInsideSeen, inside_seen);
        atomicAdd(out + kTotal, total);
        if (outside)
            atomicMin(out + kFirstBad, first_bad);
    }
};

#define GRID_STRIDE(i, n) for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (u64)gridDim.x * blockDim.x)

// binades 2^e_lo ... 2^e_hi, both signs: the first 2^20 doubles of each and 2^20 random mantissas
__global__ void binades_kernel(int e_lo, int e_hi, u64 *out)
{
    Tally t;
    const u64 per = 1ull << 21, n = (u64)(e_hi - e_lo + 1) * 2 * per;
    GRID_STRIDE(i, n) {
        const u64 j = i & (per - 1), which = i >> 21;
        const int e = e_lo + (int)(which >> 1);
        const u64 mant = j < (1ull << 20) ? j : (mix(i) & ((1ull << 52) - 1));
        const u64 bits = ((which & 1) << 63) | ((u64)(e + 1023) << 52) | mant;
        t.see(from_bits(bits));
    }
    t.flush(out);
}

// the 2^12 doubles either side of every integer i_lo ... i_hi (the integer itself included; round 0: the doubles round +-0)
__global__ void integers_kernel(int i_lo, int i_hi, u64 *out)
{
    Tally t;
    const u64 per = (1ull << 13) + 1, n = (u64)(i_hi - i_lo + 1) * per;
    GRID_STRIDE(i, n) {
        const double v = (double)(i_lo + (int)(i / per));
        const long long off = (long long)(i % per) - (1ll << 12);
        double u;
        if (v == 0.0) {  // sign-magnitude: step through the denormals on both sides of +-0
            const u64 m = (u64)(off < 0 ? -off : off);
            u = from_bits(m | (off < 0 ? 1ull << 63 : 0ull));
        } else {
            u = from_bits(to_bits(v) + (u64)(v > 0.0 ? off : -off));
        }
        t.see(u);
        if (i == 0)
            t.see(-0.0);
    }
    t.flush(out);
}

// the positions an image can produce round u = 0, through the march's own expressions: for every even size s_lo ... s_hi the
// 2^11 doubles either side of sx = -(half - 0.0001) with ux = (sx + half) - 0.0001, and of sy = half - 0.0001 with
// uy = (half - sy) - 0.0001
__global__ void reachable_kernel(int s_lo, int s_hi, u64 *out, u64 *min_nonzero)
{
    Tally t;
    double smallest = 1.0;
    const u64 per = (1ull << 12) + 1, n = (u64)((s_hi - s_lo) / 2 + 1) * per * 2;
    GRID_STRIDE(i, n) {
        const bool y_axis = (i & 1) != 0;
        const u64 k = i >> 1;
        const double half = (double)((s_lo + 2 * (int)(k / per)) / 2);
        const long long off = (long long)(k % per) - (1ll << 11);
        const double s0 = half - 0.0001;
        const double mag = from_bits(to_bits(s0) + (u64)off);
        const double u = y_axis ? (half - mag) - 0.0001 : (-mag + half) - 0.0001;
        t.see(u);
        const double m = __builtin_fabs(u);
        smallest = (m > 0.0 && m < smallest) ? m : smallest;
    }
    t.flush(out);
    atomicMin(min_nonzero, to_bits(smallest));  // (positive doubles order as their bit patterns)
}

__global__ void specials_kernel(double *w)  // +-0, +-inf, NaN: what the helper returns (w0, w1 each)
{
    const double in[5] = {0.0, -0.0, __builtin_inf(), -__builtin_inf(), __builtin_nan("")};
    if (blockIdx.x == 0 && threadIdx.x < 5)
        gcfr::bilinear_weights(in[threadIdx.x], w[2 * threadIdx.x], w[2 * threadIdx.x + 1]);
}

static bool run(const char *what, u64 *d_out, u64 h[kSlots])
{
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(h, d_out, kSlots * 8, hipMemcpyDeviceToHost) != hipSuccess)
        return false;
    std::printf("%-10s checked %12llu  in the window %10llu  mismatches outside %llu  inside %llu  first outside 0x%016llx\n", what, h[kTotal],
                h[kInsideSeen], h[kOutside], h[kInside], h[kFirstBad]);
    return true;
}

int main()
{
    u64 *d_out, *d_min;
    double *d_w;
    if (hipMalloc(&d_out, 3 * kSlots * 8) != hipSuccess || hipMalloc(&d_min, 8) != hipSuccess || hipMalloc(&d_w, 10 * 8) != hipSuccess)
        return 2;
    (void)hipMemset(d_out, 0, 3 * kSlots * 8);
    (void)hipMemset(d_min, 0x7f, 8);
    for (int k = 0; k < 3; ++k)
        (void)hipMemset(d_out + k * kSlots + kFirstBad, 0xff, 8);
    u64 h[3][kSlots];
    hipLaunchKernelGGL(binades_kernel, dim3(4096), dim3(256), 0, nullptr, -70, 12, d_out);
    hipLaunchKernelGGL(integers_kernel, dim3(2048), dim3(256), 0, nullptr, -2, 1100, d_out + kSlots);
    hipLaunchKernelGGL(reachable_kernel, dim3(2048), dim3(256), 0, nullptr, 6, 2048, d_out + 2 * kSlots, d_min);
    hipLaunchKernelGGL(specials_kernel, dim3(1), dim3(64), 0, nullptr, d_w);
    if (!run("binades", d_out, h[0]) || !run("integers", d_out + kSlots, h[1]) || !run("reachable", d_out + 2 * kSlots, h[2]))
        return 2;
    u64 h_min = 0;
    double w[10];
    if (hipMemcpy(&h_min, d_min, 8, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(w, d_w, sizeof w, hipMemcpyDeviceToHost) != hipSuccess)
        return 2;
    double smallest;
    __builtin_memcpy(&smallest, &h_min, 8);
    std::printf("reachable  smallest non-zero |u| %.3e (2^-54 = %.3e)\n", smallest, 0x1p-54);
    const char *names[5] = {"+0", "-0", "+inf", "-inf", "nan"};
    for (int k = 0; k < 5; ++k) {
        u64 b0, b1;
        __builtin_memcpy(&b0, &w[2 * k], 8);
        __builtin_memcpy(&b1, &w[2 * k + 1], 8);
        std::printf("special    u = %-4s  w0 = %g (0x%016llx)  w1 = %g (0x%016llx)\n", names[k], w[2 * k], b0, w[2 * k + 1], b1);
    }
    const u64 outside = h[0][kOutside] + h[1][kOutside] + h[2][kOutside], inside = h[0][kInside] + h[1][kInside] + h[2][kInside];
    const u64 seen = h[0][kInsideSeen] + h[1][kInsideSeen] + h[2][kInsideSeen];
    std::printf("total      mismatches outside the window %llu, inside %llu of %llu, reachable positions in the window %llu\n", outside, inside, seen,
                h[2][kInsideSeen]);
    return (outside == 0 && inside > 0 && inside == seen && h[2][kInsideSeen] == 0 && smallest > 0x1p-54) ? 0 : 1;
}

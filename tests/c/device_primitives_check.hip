// Domain sweeps of the arithmetic helpers of csrc/gcfr_device.hpp (tests/test_gpu_device_primitives.py): exp_neg,
// shadow_transfer, inv_norm3_clamped, lambert_dot, fast_rcp64, fast_sqrt64, fast_rsqrt64.  The product header is included,
// not restated; every input is made on the device from the thread index (bit patterns, or a counter-based hash with a
// fixed seed); the comparison runs on the device against f64 / IEEE references.  One line per check on stdout,
// `name key=value ...`, with the worst input; exit status 0 only if every check is inside its bound, 1 if one is not,
// 2 if a HIP call failed.  With a file name as the only argument, 64 (x, rcp, sqrt, rsqrt) records per binade are written
// there as raw f64 for the exact integer check of tests/device_primitives_reference.py.
//
// Build with the product's flags (-ffp-contract=off above all: reference chain (b.i) is a chain of separately rounded ops).
#include "../../geomconsistentfr_amd/csrc/gcfr_device.hpp"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

typedef unsigned long long u64;

#define CHECK(call)                                                                        \
    do {                                                                                   \
        const hipError_t e_ = (call);                                                      \
        if (e_ != hipSuccess) {                                                            \
            std::fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_));                \
            return 2;                                                                      \
        }                                                                                  \
    } while (0)

// ---- results: one slot per reported maximum ----
// key = (the error as f32 bits) << 32 | tag of the input (its f32 bits, or its case index): one atomicMax keeps both.  The
// f32 of the error is for the report only; `bad` counts, in f64, the inputs beyond the bound and decides the exit status.
struct Slot {
    u64 key, bad, count;
};
enum {
    A_ULP, A_SUB, A_HW, B_CHAIN, B_TANH_HELPER, B_TANH_CHAIN, B_RANGE, B_ONE, C_AXIS, C_HASH, D_ABS, D_SIGN, D_NEAR,
    E_RCP, E_SQRT, E_RSQRT, N_SLOTS
};
struct Results {
    Slot s[N_SLOTS];
    u64 hist[3][4];   // rcp / sqrt / rsqrt: inputs whose result differs by 0, 1, 2, >= 3 ulp from the IEEE one
    unsigned facts_failed, facts_run;
};

struct Acc {
    u64 key = 0, bad = 0, count = 0;
    __device__ void note(double err, double bound, unsigned tag)
    {
        ++count;
        if (!(err <= bound))
            ++bad;
        const float e = (err == err) ? (float)err : __builtin_inff();  // err >= 0: f32 bits order as the values do
        const u64 k = ((u64)__builtin_bit_cast(unsigned, e) << 32) | tag;
        key = k > key ? k : key;
    }
    __device__ void flush(Slot *s) const
    {
        if (count) {
            atomicMax(&s->key, key);
            atomicAdd(&s->count, count);
        }
        if (bad)
            atomicAdd(&s->bad, bad);
    }
};

// ---- input generators (host and device: the host turns a worst case's index back into its bits) ----
__host__ __device__ inline unsigned mix32(unsigned x)
{
    x ^= x >> 16, x *= 0x7feb352du, x ^= x >> 15, x *= 0x846ca68bu, x ^= x >> 16;
    return x;
}
__host__ __device__ inline unsigned hash(unsigned seed, unsigned i, unsigned k) { return mix32(mix32(i ^ seed) + 0x9e3779b9u * (k + 1u)); }
__host__ __device__ inline float u01(unsigned h) { return (float)(h >> 8) * 0x1p-24f; }  // [0, 1)

// (a), (b): every float from +0 to 200, then 4096 per binade up to FLT_MAX ((200, 256) included), +inf, a NaN
constexpr unsigned kBits200 = 0x43480000u;
constexpr u64 kExpDense = (u64)kBits200 + 1, kExpTail = 121ull * 4096, kExpCount = kExpDense + kExpTail + 2;
__host__ __device__ inline unsigned exp_input(u64 i)
{
    if (i < kExpDense)
        return (unsigned)i;
    i -= kExpDense;
    if (i < 4096)
        return kBits200 + 1u + (unsigned)i * 895u;  // (200, 256): up to 0x437fec82
    if (i < kExpTail)
        return ((0x86u + (unsigned)(i >> 12)) << 23) | (((unsigned)i & 4095u) << 11) | (mix32((unsigned)i) & 0x7ffu);  // 2^8 ... 2^127
    return i == kExpTail ? 0x7f800000u : 0x7fc00000u;
}

// (c): (0, 0, c), c every positive float whose square is finite (bits 1 ... 0x5f7fffff)
constexpr u64 kAxisCount = 0x5f7fffffull;
constexpr unsigned kHashCases = 1u << 24;

// (e): binades 2^-200 ... 2^200, 2^14 mantissas each (11 structured, the rest hashed), then the callers' floors
constexpr unsigned kBinades = 401, kPerBinade = 1u << 14, kF64Grid = kBinades * kPerBinade, kF64Count = kF64Grid + 3, kDumpPer = 64;
constexpr unsigned kDumpRecords = kBinades * kDumpPer + 3;
__host__ __device__ inline u64 f64_input(unsigned idx)
{
    if (idx >= kF64Grid) {
        const double floors[3] = {1e-24, 1e-12, 1e-4};  // unit_normal_from / normals_bwd_terms; the norm clamps; the 1e-4 guards
        return __builtin_bit_cast(u64, floors[idx - kF64Grid]);
    }
    const u64 ones = (1ull << 52) - 1, root2 = 0x6a09e667f3bcdull;  // sqrt(2)'s mantissa
    const unsigned j = idx % kPerBinade;
    u64 m;
    if (j < 3)
        m = j;  // 2^k and the two doubles above it
    else if (j < 6)
        m = ones - (j - 3);  // the three doubles below 2^(k+1)
    else if (j < 11)
        m = root2 + j - 8;  // sqrt(2) 2^k - 2 ulp ... + 2 ulp
    else
        m = (((u64)hash(0x0e0e0e0eu, idx, 0) << 32) | hash(0x0e0e0e0eu, idx, 1)) & ones;
    return ((u64)(idx / kPerBinade + 1023 - 200) << 52) | m;
}

__device__ inline double f32_ulp_of(double ref)  // the spacing of f32 at a normal-range |ref|
{
    const u64 ex = (__builtin_bit_cast(u64, ref) >> 52) & 0x7ffull;
    return __builtin_bit_cast(double, (ex - 23) << 52);
}

// ---- (a) exp_neg, (b) shadow_transfer ----
__global__ __launch_bounds__(256) void exp_kernel(Results *res)
{
    Acc a_ulp, a_sub, a_hw, b_chain, b_th, b_tc, b_range, b_one;
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < kExpCount; i += stride) {
        const unsigned bits = exp_input(i);
        const float d = __builtin_bit_cast(float, bits);
        const float g = gcfr::exp_neg(d), w = gcfr::shadow_transfer(d);
        if (d != d) {  // NaN in, NaN out (both)
            a_ulp.note((g != g) ? 0.0 : __builtin_inf(), 2.0, bits);
            b_chain.note((w != w) ? 0.0 : __builtin_inf(), 1e-6, bits);
            continue;
        }
        const double ref = exp(-(double)d);
        // (a) where the reference is a normal f32: the error in ulps of the reference; below 2^-126 the absolute error, where
        // up to 2^-126 is allowed -- v_exp_f32 and the f32 arithmetic after it may flush a denormal result to zero
        if (ref >= 0x1p-126)
            a_ulp.note(fabs((double)g - ref) / f32_ulp_of(ref), 2.0, bits);
        else
            a_sub.note(fabs((double)g - ref), 0x1p-126, bits);
        {  // what the hardware's 2^t delivers alone, on exp_neg's own argument (report only)
            const float t = -((d > 200.0f) ? 200.0f : d) * 1.44269502e+0f;
            const double r2 = exp2((double)t);
            if (r2 >= 0x1p-126)
                a_hw.note(fabs((double)__builtin_amdgcn_exp2f(t) - r2) / f32_ulp_of(r2), __builtin_inf(), bits);
        }
        // (b.i) the oracle's chain (oracle/gcfr_oracle.c, shadow transfer) in IEEE f32 on the rounded f64 exponential
        const float e = (float)ref;
        const float onepe = 1.0f + e;
        const float chain = (-4.0f * e) / (onepe * onepe) + 1.0f;
        b_chain.note(fabs((double)w - (double)chain), 1e-6, bits);
        // (b.ii) tanh^2(d/2) in f64: how much of the distance is the formula's own cancellation (report only)
        const double th = tanh(0.5 * (double)d), t2 = th * th;
        b_th.note(fabs((double)w - t2), __builtin_inf(), bits);
        b_tc.note(fabs((double)chain - t2), __builtin_inf(), bits);
        // -1e-6 <= w <= 1 everywhere; w == 1 from d = 40 on
        b_range.note((w <= 1.0f && (double)w >= -1e-6) ? 0.0 : 1.0, 0.5, bits);
        if (d >= 40.0f)
            b_one.note(w == 1.0f ? 0.0 : 1.0, 0.5, bits);
    }
    a_ulp.flush(&res->s[A_ULP]), a_sub.flush(&res->s[A_SUB]), a_hw.flush(&res->s[A_HW]), b_chain.flush(&res->s[B_CHAIN]);
    b_th.flush(&res->s[B_TANH_HELPER]), b_tc.flush(&res->s[B_TANH_CHAIN]), b_range.flush(&res->s[B_RANGE]), b_one.flush(&res->s[B_ONE]);
}

// ---- (c) inv_norm3_clamped ----
__device__ inline double inv_norm_error(float a, float b, float c)
{
    const float s2 = __builtin_fmaf(c, c, __builtin_fmaf(b, b, a * a));  // the helper's own order: the reference starts from ITS s2
    const double n = __builtin_sqrt((double)s2), ref = 1.0 / (n > 1e-12 ? n : 1e-12);
    return fabs((double)gcfr::inv_norm3_clamped(a, b, c) - ref) / ref;
}
constexpr double kInvNormBound = 3.0 * 0x1p-24;
__global__ __launch_bounds__(256) void inv_norm_axis_kernel(Results *res)
{
    Acc acc;
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < kAxisCount; i += stride) {
        const unsigned bits = 1u + (unsigned)i;
        acc.note(inv_norm_error(0.0f, 0.0f, __builtin_bit_cast(float, bits)), kInvNormBound, bits);
    }
    acc.flush(&res->s[C_AXIS]);
}
__global__ __launch_bounds__(256) void inv_norm_hash_kernel(Results *res)
{
    Acc acc;
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < kHashCases) {
        const unsigned seed = 0xc0c0c0c0u;
        const float mag = exp10f(-13.0f + 31.0f * u01(hash(seed, i, 0)));  // 1e-13 ... 1e18, log-uniform
        const float a = mag * (2.0f * u01(hash(seed, i, 1)) - 1.0f), b = mag * (2.0f * u01(hash(seed, i, 2)) - 1.0f);
        const float c = mag * (2.0f * u01(hash(seed, i, 3)) - 1.0f);
        acc.note(inv_norm_error(a, b, c), kInvNormBound, i);
    }
    acc.flush(&res->s[C_HASH]);
}

// ---- (d) lambert_dot, in the shapes of the project's scenes ----
__global__ __launch_bounds__(256) void lambert_kernel(Results *res)
{
    Acc d_abs, d_sign, d_near;
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < kHashCases) {
        const unsigned seed = 0xd0d0d0d0u;
        const float x = (float)((int)(hash(seed, i, 0) % 513u) - 256), y = (float)((int)(hash(seed, i, 1) % 513u) - 256);
        const float zb = 60.0f * sqrtf(-2.0f * logf(1.0f - u01(hash(seed, i, 2)))) * cospif(2.0f * u01(hash(seed, i, 3)));
        const float dists[4] = {8.0f, 30.0f, 60.0f, 4013.0f};  // tests/test_gpu_configs.py
        const float dist = dists[i & 3u];
        // light direction: uniform on the upper half sphere
        const float cz = u01(hash(seed, i, 4)), cr = sqrtf(1.0f - cz * cz), cphi = 2.0f * u01(hash(seed, i, 5));
        const float Cx = dist * cr * cospif(cphi), Cy = dist * cr * sinpif(cphi), Cz = dist * cz;
        // normal: any direction, length 1e-6 ... 1e6
        const double len = exp10(-6.0 + 12.0 * (double)u01(hash(seed, i, 6)));
        const double vz = 2.0 * (double)u01(hash(seed, i, 7)) - 1.0, vr = sqrt(1.0 - vz * vz), vphi = 2.0 * (double)u01(hash(seed, i, 8));
        double v0 = vr * cospi(vphi), v1 = vr * sinpi(vphi), v2 = vz;
        const bool near_kink = ((i >> 2) & 3u) == 0;  // a quarter of the cases, for every light distance
        if (near_kink) {  // into the plane perpendicular to the light direction, then a tilt: the exact dot within 2e-4 of zero
            const double lx = (double)(Cx - x), ly = (double)(Cy - y), lz = (double)(Cz - zb);
            const double rl = 1.0 / sqrt(lx * lx + ly * ly + lz * lz + 1e-300);
            const double u0 = lx * rl, u1 = ly * rl, u2 = lz * rl;
            const double p = v0 * u0 + v1 * u1 + v2 * u2;
            v0 -= p * u0, v1 -= p * u1, v2 -= p * u2;
            const double rv = 1.0 / sqrt(v0 * v0 + v1 * v1 + v2 * v2 + 1e-300);
            const double tilt = 2e-4 * (2.0 * (double)u01(hash(seed, i, 9)) - 1.0);
            v0 = v0 * rv + tilt * u0, v1 = v1 * rv + tilt * u1, v2 = v2 * rv + tilt * u2;
        }
        const float nx = (float)(len * v0), ny = (float)(len * v1), nz = (float)(len * v2);
        // reference: l in f32 as the forward forms it, everything after it in f64
        const double lx = (double)(Cx - x), ly = (double)(Cy - y), lz = (double)(Cz - zb);
        const double ln = __builtin_sqrt(lx * lx + ly * ly + lz * lz), nn = __builtin_sqrt((double)nx * nx + (double)ny * ny + (double)nz * nz);
        const double il = 1.0 / (ln > 1e-12 ? ln : 1e-12), in = 1.0 / (nn > 1e-12 ? nn : 1e-12);
        const double ref = (nx * in) * (lx * il) + (ny * in) * (ly * il) + (nz * in) * (lz * il);
        const float got = gcfr::lambert_dot(x, y, zb, nx, ny, nz, Cx, Cy, Cz);
        d_abs.note(fabs((double)got - ref), 1e-6, i);
        if (fabs(ref) >= 1e-4)  // the kink rule of the backward kernels: outside their window the forward has the exact sign
            d_sign.note(((ref > 0.0) ? (got > 0.0f) : (got < 0.0f)) ? 0.0 : 1.0, 0.5, i);
        if (near_kink)
            d_near.note(fabs(ref), 2.01e-4, i);  // the construction itself: these cases are where it says they are
    }
    d_abs.flush(&res->s[D_ABS]), d_sign.flush(&res->s[D_SIGN]), d_near.flush(&res->s[D_NEAR]);
}

// ---- (e) fast_rcp64, fast_sqrt64, fast_rsqrt64 against the IEEE operations ----
__device__ inline double ulps_apart(double a, double b)  // same sign, finite: the distance of the bit patterns
{
    if (a != a || b != b)
        return (a != a && b != b) ? 0.0 : __builtin_inf();
    const long long d = (long long)__builtin_bit_cast(u64, a) - (long long)__builtin_bit_cast(u64, b);
    return (double)(d < 0 ? -d : d);
}
__global__ __launch_bounds__(256) void f64_kernel(Results *res, double *dump)
{
    Acc rcp, sq, rsq;
    u64 h[3][4] = {};
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < kF64Count) {
        const double x = __builtin_bit_cast(double, f64_input(i));
        const double r = gcfr::fast_rcp64(x), rn = gcfr::fast_rcp64(-x), s = gcfr::fast_sqrt64(x), q = gcfr::fast_rsqrt64(x);
        const double root = __builtin_sqrt(x);
        const double d_r = ulps_apart(r, 1.0 / x), d_rn = ulps_apart(rn, 1.0 / -x), d_s = ulps_apart(s, root), d_q = ulps_apart(q, 1.0 / root);
        rcp.note(d_r, 1.0, i), rcp.note(d_rn, 1.0, i | 0x80000000u), sq.note(d_s, 1.0, i), rsq.note(d_q, 2.0, i);
        ++h[0][d_r < 3.0 ? (int)d_r : 3], ++h[0][d_rn < 3.0 ? (int)d_rn : 3], ++h[1][d_s < 3.0 ? (int)d_s : 3], ++h[2][d_q < 3.0 ? (int)d_q : 3];
        const unsigned j = i % kPerBinade;
        if (i >= kF64Grid || j < kDumpPer) {
            const unsigned rec = i >= kF64Grid ? kBinades * kDumpPer + (i - kF64Grid) : (i / kPerBinade) * kDumpPer + j;  // < kDumpRecords
            dump[rec * 4 + 0] = x, dump[rec * 4 + 1] = r, dump[rec * 4 + 2] = s, dump[rec * 4 + 3] = q;
        }
    }
    rcp.flush(&res->s[E_RCP]), sq.flush(&res->s[E_SQRT]), rsq.flush(&res->s[E_RSQRT]);
    for (int k = 0; k < 3; ++k)
        for (int b = 0; b < 4; ++b)
            if (h[k][b])
                atomicAdd(&res->hist[k][b], h[k][b]);
}

// ---- exact facts: one thread each, inputs from a table indexed by the thread (nothing for the compiler to fold) ----
__device__ const unsigned kFactBits[8] = {0x00000000u /* 0 */, 0x7f800000u /* +inf */, 0x7fc00000u /* NaN */, 0x49742400u /* 1e6 */,
                                          0x5f800000u /* 2^64 */, 0x3f800000u /* 1 */, 0x179abe15u /* 1e-24f */, 0x2b8cbcccu /* 1e-12f */};
__global__ void facts_kernel(Results *res)
{
    const unsigned t = threadIdx.x;
    const float zero = __builtin_bit_cast(float, kFactBits[0]), inf = __builtin_bit_cast(float, kFactBits[1]);
    const float nan = __builtin_bit_cast(float, kFactBits[2]), one = __builtin_bit_cast(float, kFactBits[5]);
    bool ok = true;
    switch (t) {
    case 0: ok = gcfr::exp_neg(zero) == 1.0f; break;
    case 1: ok = gcfr::exp_neg(inf) == 0.0f; break;
    case 2: { const float g = gcfr::exp_neg(nan); ok = g != g; break; }
    case 3: ok = gcfr::shadow_transfer(zero) == 0.0f; break;
    case 4: ok = gcfr::shadow_transfer(__builtin_bit_cast(float, kFactBits[3])) == 1.0f && __builtin_bit_cast(float, kFactBits[3]) == gcfr::kMaskedDistance; break;
    case 5: ok = gcfr::shadow_transfer(inf) == 1.0f; break;
    case 6: { const float w = gcfr::shadow_transfer(nan); ok = w != w; break; }
    case 7: ok = gcfr::inv_norm3_clamped(zero, zero, zero) == 1e12f; break;
    case 8: {  // a NaN component: the clamp's value comes back, and the PRODUCT is NaN
        const float r = gcfr::inv_norm3_clamped(nan, one, one), p = nan * r;
        ok = r == 1e12f && p != p;
        break;
    }
    case 9: {  // |v|^2 = +inf gives NaN (documented in the helper's comment; sqrt-then-divide would give 0)
        const float r = gcfr::inv_norm3_clamped(zero, zero, __builtin_bit_cast(float, kFactBits[4]));
        ok = r != r;
        break;
    }
    case 10: case 11: case 12: {  // s2 == 1e-24f and its two neighbours: at or below the floor the clamp, above it the reciprocal norm
        const unsigned target = kFactBits[6] + t - 11u;
        bool found = false;
        for (int dc = -16; dc <= 16 && !found; ++dc)
            for (int j = 0; j <= 64 && !found; ++j) {
                const float c = __builtin_bit_cast(float, kFactBits[7] + (unsigned)dc), b = (float)j * 0x1p-55f;
                const float s2 = __builtin_fmaf(c, c, __builtin_fmaf(b, b, zero * zero));
                if (__builtin_bit_cast(unsigned, s2) != target)
                    continue;
                found = true;
                const float r = gcfr::inv_norm3_clamped(zero, b, c);
                ok = (t == 12) ? (r != 1e12f && inv_norm_error(zero, b, c) <= kInvNormBound) : (r == 1e12f);
            }
        ok = ok && found;
        break;
    }
    default: return;
    }
    atomicAdd(&res->facts_run, 1u);
    if (!ok)
        atomicOr(&res->facts_failed, 1u << t);
}
constexpr unsigned kFacts = 13;

static double key_err(u64 key) { const unsigned b = (unsigned)(key >> 32); float f; std::memcpy(&f, &b, 4); return (double)f; }
static unsigned key_tag(u64 key) { return (unsigned)key; }

int main(int argc, char **argv)
{
    Results *res;
    double *dump;
    CHECK(hipMalloc(&res, sizeof(Results)));
    CHECK(hipMemset(res, 0, sizeof(Results)));
    CHECK(hipMalloc(&dump, sizeof(double) * 4 * kDumpRecords));
    CHECK(hipMemset(dump, 0, sizeof(double) * 4 * kDumpRecords));
    double secs[6];
    int n = 0;
#define RUN(kernel, blocks, ...)                                                                     \
    do {                                                                                             \
        const auto t0 = std::chrono::steady_clock::now();                                            \
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, nullptr, __VA_ARGS__);                \
        CHECK(hipGetLastError());                                                                    \
        CHECK(hipDeviceSynchronize());                                                               \
        secs[n++] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();    \
    } while (0)
    RUN(exp_kernel, 2048, res);
    RUN(inv_norm_axis_kernel, 2048, res);
    RUN(inv_norm_hash_kernel, kHashCases / 256, res);
    RUN(lambert_kernel, kHashCases / 256, res);
    RUN(f64_kernel, (kF64Count + 255) / 256, res, dump);
    hipLaunchKernelGGL(facts_kernel, dim3(1), dim3(64), 0, nullptr, res);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    Results h;
    CHECK(hipMemcpy(&h, res, sizeof(Results), hipMemcpyDeviceToHost));
    std::vector<double> rec(4 * (size_t)kDumpRecords);
    CHECK(hipMemcpy(rec.data(), dump, sizeof(double) * rec.size(), hipMemcpyDeviceToHost));
    CHECK(hipFree(res));
    CHECK(hipFree(dump));

    const Slot *s = h.s;
    std::printf("exp_neg count=%llu max_ulp=%.6g worst=0x%08x bad=%llu bound=2 seconds=%.3f\n", s[A_ULP].count + s[A_SUB].count,
                key_err(s[A_ULP].key), key_tag(s[A_ULP].key), s[A_ULP].bad, secs[0]);
    std::printf("exp_neg_below_normal count=%llu max_abs=%.6g worst=0x%08x bad=%llu bound=%.9g\n", s[A_SUB].count, key_err(s[A_SUB].key),
                key_tag(s[A_SUB].key), s[A_SUB].bad, 0x1p-126);
    std::printf("v_exp_f32 count=%llu max_ulp=%.6g worst=0x%08x\n", s[A_HW].count, key_err(s[A_HW].key), key_tag(s[A_HW].key));
    std::printf("shadow_transfer count=%llu max_abs=%.6g worst=0x%08x bad=%llu bound=1e-6\n", s[B_CHAIN].count, key_err(s[B_CHAIN].key),
                key_tag(s[B_CHAIN].key), s[B_CHAIN].bad);
    std::printf("shadow_transfer_tanh2 count=%llu helper_max_abs=%.6g helper_worst=0x%08x chain_max_abs=%.6g chain_worst=0x%08x\n",
                s[B_TANH_HELPER].count, key_err(s[B_TANH_HELPER].key), key_tag(s[B_TANH_HELPER].key), key_err(s[B_TANH_CHAIN].key),
                key_tag(s[B_TANH_CHAIN].key));
    std::printf("shadow_transfer_range count=%llu bad=%llu worst=0x%08x from40_count=%llu from40_bad=%llu from40_worst=0x%08x\n", s[B_RANGE].count,
                s[B_RANGE].bad, key_tag(s[B_RANGE].key), s[B_ONE].count, s[B_ONE].bad, key_tag(s[B_ONE].key));
    std::printf("inv_norm3_axis count=%llu max_rel=%.6g worst=0x%08x bad=%llu bound=%.9g seconds=%.3f\n", s[C_AXIS].count, key_err(s[C_AXIS].key),
                key_tag(s[C_AXIS].key), s[C_AXIS].bad, kInvNormBound, secs[1]);
    std::printf("inv_norm3_hashed count=%llu max_rel=%.6g worst_case=%u bad=%llu bound=%.9g seconds=%.3f\n", s[C_HASH].count,
                key_err(s[C_HASH].key), key_tag(s[C_HASH].key), s[C_HASH].bad, kInvNormBound, secs[2]);
    std::printf("lambert_dot count=%llu max_abs=%.6g worst_case=%u bad=%llu bound=1e-6 seconds=%.3f\n", s[D_ABS].count, key_err(s[D_ABS].key),
                key_tag(s[D_ABS].key), s[D_ABS].bad, secs[3]);
    std::printf("lambert_dot_sign count=%llu bad=%llu worst_case=%u near_kink_count=%llu near_kink_max_abs_dot=%.6g near_kink_bad=%llu\n",
                s[D_SIGN].count, s[D_SIGN].bad, key_tag(s[D_SIGN].key), s[D_NEAR].count, key_err(s[D_NEAR].key), s[D_NEAR].bad);
    const char *names[3] = {"fast_rcp64", "fast_sqrt64", "fast_rsqrt64"};
    for (int k = 0; k < 3; ++k) {
        const Slot &e = s[E_RCP + k];
        const unsigned tag = key_tag(e.key);
        u64 xb = f64_input(tag & 0x7fffffffu);
        if (tag & 0x80000000u)
            xb |= 1ull << 63;
        std::printf("%s count=%llu max_ulp=%.6g worst=0x%016llx bad=%llu bound=%d ulp0=%llu ulp1=%llu ulp2=%llu ulp3plus=%llu seconds=%.3f\n", names[k],
                    e.count, key_err(e.key), xb, e.bad, k == 2 ? 2 : 1, h.hist[k][0], h.hist[k][1], h.hist[k][2], h.hist[k][3], secs[4]);
    }
    std::printf("facts count=%u failed=0x%x\n", h.facts_run, h.facts_failed);
    if (argc > 1) {
        std::FILE *f = std::fopen(argv[1], "wb");
        if (!f || std::fwrite(rec.data(), sizeof(double), rec.size(), f) != rec.size() || std::fclose(f) != 0) {
            std::fprintf(stderr, "cannot write %s\n", argv[1]);
            return 2;
        }
        std::printf("dump records=%u\n", kDumpRecords);
    }
    u64 bad = h.facts_failed || h.facts_run != kFacts;
    for (int k = 0; k < N_SLOTS; ++k)
        bad += s[k].bad;
    return bad ? 1 : 0;
}

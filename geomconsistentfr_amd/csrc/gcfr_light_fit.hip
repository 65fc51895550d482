// Rig capture, gfx950: the colours x weights `rgb` (L,3) of a light rig fitted to a photograph by weighted least squares over the
// per-light shadings of the many-lights path -- the inverse of the light-rig stage (gcfr_light_rig.hip):
//
//     image[b,c,p] ~ albedo[b,c,p] sum_l x[b,l,c] final[b,l,p]        G_c[l,l'] = sum_p w a_c^2 f_l f_l'      r_c[l] = sum_p w a_c I_c f_l
//
// Three kernels per fit, no floating-point atomic, no cross-lane reduction, every sum in f64 in a FIXED order (include/gcfr.h):
//
//   partials   a workgroup of 256 lanes owns one face and walks that face's chunks of kFitChunk pixels j, j + groups, ... ascending.
//              Per chunk it stages in LDS the L rows of `final` (f32, row stride kFitStride floats) and, per channel, q = (w a) a and
//              u = (w a) I in f64.  Lanes own ENTRIES, not pixels: per channel the L (L + 1) / 2 entries of G's lower triangle and the L
//              of r, enumerated row by row as (l, 0), ..., (l, l), (l, r); entry e belongs to lane e mod 256, slot e / 256, and lives in
//              a register for the whole launch (at L = 64: 3 x 2144 = 6432 entries, 26 slots).  Per pixel, ascending, an entry adds
//              (s f_l) f_j with s = q and j = l' for G, s = u and j = a row of ones for r -- (u f_l) 1.0 is u f_l exactly, so the two
//              kinds of entry run the same instructions.  Adjacent lanes read the same s and f_l (a broadcast) and adjacent rows l'
//              at one pixel: with kFitStride = 65 floats these are 32 different banks for a half wave.
//   finish     one lane per (face, entry): the face's partials added in ascending workgroup order, starting from partial 0; G written
//              full (the upper triangle a copy), r beside it.
//   solve      one workgroup of 64 lanes (one wave) per (rig, channel): the faces' systems added in ascending b (one shared rig),
//              the ridge, a left-looking Cholesky factorisation in LDS with lane i owning row i, forward and back substitution; one
//              rounding to f32.
//   non-negative solve   the same system under x >= 0 by an active-set method: the same factorisation restricted to the lights of
//              the passive set, once per step, in place of `solve`.
//
// Work per pixel and channel at L lights, N = L (L + 3) / 2 entries: 3 N f64 operations (two products, one sum) + 2 N conversions
// f32 -> f64, 3 N LDS reads (8 + 4 + 4 bytes); from memory 4 L + 28 bytes per pixel (final, albedo, image, weight), once.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/gcfr.h"

namespace gcfr {

constexpr int kFitLanes = 256;
constexpr int kFitChunk = 64;                  // pixels per chunk (lighting.LIGHT_FIT_CHUNK mirrors it)
constexpr int kFitStride = kFitChunk + 1;      // floats per staged row of `final`
constexpr int kFitMaxGroups = 512;             // workgroups per launch at the most, two per CU (lighting.LIGHT_FIT_MAX_GROUPS)
constexpr int kFitMaxLights = 64;
constexpr int kFitMaxFaces = 65535;            // B rides in blockIdx.y
constexpr int kSolveLanes = 64;

inline uint32_t fit_entries(uint32_t L) { return 3u * (L * (L + 3u) / 2u); }

inline uint32_t fit_groups(uint32_t B, uint32_t HW)
{
    const uint32_t chunks = (HW + (uint32_t)kFitChunk - 1u) / (uint32_t)kFitChunk;
    uint32_t cap = (uint32_t)kFitMaxGroups / B;
    if (cap < 1u)
        cap = 1u;
    return chunks < cap ? chunks : cap;
}

inline bool fit_shape_ok(int32_t B, int32_t L, int32_t H, int32_t W)
{
    if (B < 1 || B > kFitMaxFaces || L < 1 || L > kFitMaxLights || H < 1 || W < 1)
        return false;
    return (uint64_t)H * (uint64_t)W < (1ull << 31) - (uint64_t)kFitChunk;
}

// SLOTS: entries per lane, >= ceil(3 N / 256); a slot past the last entry computes on entry 0's addresses and is not stored
template <int SLOTS>
__global__ __launch_bounds__(kFitLanes) void light_fit_partials_kernel(
    const float *__restrict__ final_shading, const float *__restrict__ albedo, const float *__restrict__ image, int image_nhwc,
    const float *__restrict__ weight, int weight_per_face, uint32_t L, uint32_t HW, uint32_t n_entries, double *__restrict__ partials)
{
    __shared__ float rows[(kFitMaxLights + 1) * kFitStride];        // row L: ones
    __shared__ double qu[6 * kFitChunk];                            // q of channels 0 .. 2, then u of channels 0 .. 2
    const uint32_t lane = threadIdx.x, group = blockIdx.x, groups = gridDim.x, b = blockIdx.y;
    const uint32_t per_channel = L * (L + 3u) / 2u;

    // which (s, f_l, f_j) each of this lane's entries reads, as LDS offsets
    uint32_t off_s[SLOTS], off_l[SLOTS], off_j[SLOTS];
#pragma unroll
    for (int k = 0; k < SLOTS; ++k) {
        uint32_t e = lane + (uint32_t)kFitLanes * (uint32_t)k;
        if (e >= n_entries)
            e = 0u;
        const uint32_t c = e / per_channel, r = e - c * per_channel;
        uint32_t l = (uint32_t)((sqrtf(8.0f * (float)r + 9.0f) - 3.0f) * 0.5f);          // row l starts at l (l + 3) / 2
        while (l > 0u && l * (l + 3u) / 2u > r)
            --l;
        while ((l + 1u) * (l + 4u) / 2u <= r)
            ++l;
        const uint32_t j = r - l * (l + 3u) / 2u;                                        // 0 .. l: G[l,j];  l + 1: r[l]
        const bool is_rhs = j == l + 1u;
        off_s[k] = ((is_rhs ? 3u : 0u) + c) * (uint32_t)kFitChunk;
        off_l[k] = l * (uint32_t)kFitStride;
        off_j[k] = (is_rhs ? L : j) * (uint32_t)kFitStride;
    }
    double acc[SLOTS];
#pragma unroll
    for (int k = 0; k < SLOTS; ++k)
        acc[k] = 0.0;
    for (uint32_t i = lane; i < (uint32_t)kFitChunk; i += (uint32_t)kFitLanes)
        rows[L * (uint32_t)kFitStride + i] = 1.0f;

    const uint32_t chunks = (HW + (uint32_t)kFitChunk - 1u) / (uint32_t)kFitChunk;
    const float *face_final = final_shading + (size_t)b * L * HW;
    const float *face_albedo = albedo + (size_t)b * 3u * HW;
    const float *face_image = image + (size_t)b * 3u * HW;
    const float *face_weight = weight ? weight + (weight_per_face ? (size_t)b * HW : (size_t)0) : nullptr;
    for (uint32_t chunk = group; chunk < chunks; chunk += groups) {                      // (uniform)
        const uint32_t start = chunk * (uint32_t)kFitChunk;
        const uint32_t n = HW - start < (uint32_t)kFitChunk ? HW - start : (uint32_t)kFitChunk;
        __syncthreads();                                                                 // the previous chunk has been read
        for (uint32_t i = lane; i < L * (uint32_t)kFitChunk; i += (uint32_t)kFitLanes) {
            const uint32_t l = i / (uint32_t)kFitChunk, p = i - l * (uint32_t)kFitChunk;
            if (p < n)
                rows[l * (uint32_t)kFitStride + p] = face_final[(size_t)l * HW + start + p];
        }
        if (lane < 3u * (uint32_t)kFitChunk) {
            const uint32_t c = lane / (uint32_t)kFitChunk, p = lane - c * (uint32_t)kFitChunk;
            if (p < n) {
                const uint32_t pix = start + p;
                const float w = face_weight ? face_weight[pix] : 1.0f;
                const float a = face_albedo[(size_t)c * HW + pix];
                const float im = image_nhwc ? face_image[(size_t)pix * 3u + c] : face_image[(size_t)c * HW + pix];
                const double s = (double)w * (double)a;
                qu[c * (uint32_t)kFitChunk + p] = s * (double)a;
                qu[(3u + c) * (uint32_t)kFitChunk + p] = s * (double)im;
            }
        }
        __syncthreads();
#pragma unroll 2
        for (uint32_t p = 0; p < n; ++p) {
#pragma unroll
            for (int k = 0; k < SLOTS; ++k)
                acc[k] = acc[k] + (qu[off_s[k] + p] * (double)rows[off_l[k] + p]) * (double)rows[off_j[k] + p];
        }
    }
    double *mine = partials + ((size_t)b * groups + group) * n_entries;
#pragma unroll
    for (int k = 0; k < SLOTS; ++k) {
        const uint32_t e = lane + (uint32_t)kFitLanes * (uint32_t)k;
        if (e < n_entries)
            mine[e] = acc[k];
    }
}

__global__ __launch_bounds__(kFitLanes) void light_fit_finish_kernel(const double *__restrict__ partials, uint32_t groups, uint32_t L,
                                                                     uint32_t n_entries, double *__restrict__ gram,
                                                                     double *__restrict__ rhs)
{
    const uint32_t e = blockIdx.x * (uint32_t)kFitLanes + threadIdx.x, b = blockIdx.y;
    if (e >= n_entries)
        return;
    const double *p = partials + (size_t)b * groups * n_entries + e;
    double total = p[0];
    for (uint32_t g = 1; g < groups; ++g)
        total = total + p[(size_t)g * n_entries];
    const uint32_t per_channel = L * (L + 3u) / 2u;
    const uint32_t c = e / per_channel, r = e - c * per_channel;
    uint32_t l = 0;
    while ((l + 1u) * (l + 4u) / 2u <= r)
        ++l;
    const uint32_t j = r - l * (l + 3u) / 2u;
    if (j == l + 1u) {
        rhs[((size_t)b * 3u + c) * L + l] = total;
    } else {
        double *G = gram + ((size_t)b * 3u + c) * L * L;
        G[(size_t)l * L + j] = total;
        G[(size_t)j * L + l] = total;
    }
}

constexpr uint32_t kSolveStride = (uint32_t)kFitMaxLights + 1u;   // row stride in doubles: lanes reading one column hit 32 banks

// Both solves start here.  Lane i < L: the lower triangle of row i of the summed system (faces in ascending b) into A, the relative
// ridge on its diagonal; -> the summed right-hand side r_i (0 for a lane without a row).  Ends behind a barrier.
__device__ __forceinline__ double fit_load_system(const double *__restrict__ gram, const double *__restrict__ rhs, uint32_t B, uint32_t L,
                                                  double ridge, uint32_t rgb_batch, uint32_t c, uint32_t rig, double *A, double *shift)
{
    constexpr uint32_t S = kSolveStride;
    const uint32_t i = threadIdx.x;
    const uint32_t faces = rgb_batch == 1u ? B : 1u, first = rgb_batch == 1u ? 0u : rig;
    const bool row = i < L;
    double y = 0.0;
    if (row) {
        for (uint32_t j = 0; j <= i; ++j) {
            double s = gram[(((size_t)first * 3u + c) * L + i) * L + j];
            for (uint32_t f = 1; f < faces; ++f)
                s = s + gram[(((size_t)(first + f) * 3u + c) * L + i) * L + j];
            A[i * S + j] = s;
        }
        y = rhs[((size_t)first * 3u + c) * L + i];
        for (uint32_t f = 1; f < faces; ++f)
            y = y + rhs[((size_t)(first + f) * 3u + c) * L + i];
    }
    __syncthreads();
    if (i == 0u) {
        double trace = 0.0;
        for (uint32_t l = 0; l < L; ++l)
            trace = trace + A[l * S + l];
        *shift = ridge * (trace / (double)L);
    }
    __syncthreads();
    if (row)
        A[i * S + i] = A[i * S + i] + *shift;
    __syncthreads();
    return y;
}

// Lane i owns row i.  A holds the system's lower triangle, then the factor's strictly lower triangle; `diag` the factor's diagonal.
__global__ __launch_bounds__(kSolveLanes) void light_fit_solve_kernel(const double *__restrict__ gram, const double *__restrict__ rhs,
                                                                      uint32_t B, uint32_t L, double ridge, uint32_t rgb_batch,
                                                                      float *__restrict__ rgb, int32_t *__restrict__ info)
{
    constexpr uint32_t S = kSolveStride;
    __shared__ double A[kFitMaxLights * (kFitMaxLights + 1)];
    __shared__ double diag[kFitMaxLights];
    __shared__ double piv[kFitMaxLights];
    __shared__ double sol[kFitMaxLights];
    __shared__ double shift;
    const uint32_t i = threadIdx.x, c = blockIdx.x, rig = blockIdx.y;
    const bool row = i < L;
    double y = fit_load_system(gram, rhs, B, L, ridge, rgb_batch, c, rig, A, &shift);

    int32_t bad = 0;
    for (uint32_t k = 0; k < L; ++k) {                               // (uniform)
        double s = 0.0;
        if (row && i >= k) {
            s = A[i * S + k];
            for (uint32_t m = 0; m < k; ++m)
                s = s - A[i * S + m] * A[k * S + m];
            if (i == k)
                piv[k] = s;
        }
        __syncthreads();
        const double pk = piv[k];
        if (!(pk > 0.0 && pk < __builtin_huge_val())) {              // not a positive finite number (a NaN fails both)
            bad = (int32_t)k + 1;
            break;
        }
        const double d = sqrt(pk);
        if (i == k)
            diag[k] = d;
        else if (row && i > k)
            A[i * S + k] = s / d;
        __syncthreads();
    }
    float *out = rgb + (size_t)rig * L * 3u + c;
    if (bad) {
        if (row)
            out[(size_t)i * 3u] = __builtin_nanf("");
        if (i == 0u)
            info[rig * 3u + c] = bad;
        return;
    }
    for (uint32_t k = 0; k < L; ++k) {                               // L z = y, column by column
        if (i == k)
            sol[k] = y / diag[k];
        __syncthreads();
        if (row && i > k)
            y = y - A[i * S + k] * sol[k];
    }
    if (row)
        y = sol[i];
    __syncthreads();
    for (uint32_t k = L; k-- > 0u;) {                                // L^T x = z, from the last column
        if (i == k)
            sol[k] = y / diag[k];
        __syncthreads();
        if (i < k)
            y = y - A[k * S + i] * sol[k];
    }
    if (row)
        out[(size_t)i * 3u] = (float)sol[i];
    if (i == 0u)
        info[rig * 3u + c] = 0;
}

// The non-negative solve (include/gcfr.h states the order): Lawson and Hanson's active-set method on the normal equations.  Lane i
// owns light i -- its r_i, x_i, s_i, w_i are registers; the passive set P is a wave-uniform 64-bit mask and every loop over it a
// scalar loop over its set bits.  A's lower triangle (the system) stays intact: A[i,j] for j > i is read as A[j,i].  The factor's
// strictly lower triangle lives TRANSPOSED in A's unused upper triangle, C[i,m] at A[m * S + i] for i > m (lanes reading one column
// of C read consecutive doubles), its diagonal in `diag`.
__global__ __launch_bounds__(kSolveLanes) void light_fit_solve_nonneg_kernel(const double *__restrict__ gram,
                                                                             const double *__restrict__ rhs, uint32_t B, uint32_t L,
                                                                             double ridge, uint32_t rgb_batch, uint32_t cap,
                                                                             float *__restrict__ rgb, int32_t *__restrict__ info,
                                                                             int32_t *__restrict__ solves)
{
    constexpr uint32_t S = kSolveStride;
    __shared__ double A[kFitMaxLights * (kFitMaxLights + 1)];
    __shared__ double diag[kFitMaxLights];
    __shared__ double sol[kFitMaxLights];
    __shared__ double xs[kFitMaxLights];                             // x, for the other lanes' w
    __shared__ double lane_val[kFitMaxLights];                       // r, then w or the step quotients: what arg-max / arg-min read
    __shared__ double piv;
    __shared__ double shift;
    const uint32_t i = threadIdx.x, c = blockIdx.x, rig = blockIdx.y;
    const bool row = i < L;
    const double r = fit_load_system(gram, rhs, B, L, ridge, rgb_batch, c, rig, A, &shift);
    lane_val[i] = r;
    xs[i] = 0.0;
    __syncthreads();
    double largest = 0.0;
    for (uint32_t l = 0; l < L; ++l) {                               // (uniform; a NaN never enters)
        const double v = fabs(lane_val[l]);
        largest = v > largest ? v : largest;
    }
    const double tol = 0x1p-40 * largest;
    __syncthreads();

    uint64_t P = 0;                                                  // (uniform)
    double x = 0.0;
    uint32_t n = 0;
    int32_t status = -1;                                             // the cap, unless step 2 finds nothing to admit
    for (uint32_t outer = 0; outer <= cap; ++outer) {                // every outer step that goes on has factorised: it ends by `break`
        // 2. the gradient of the lights outside P, the largest one enters
        double w = r;
        for (uint64_t m = P; m; m &= m - 1) {
            const uint32_t j = (uint32_t)__builtin_ctzll(m);
            w = w - A[j <= i ? i * S + j : j * S + i] * xs[j];
        }
        lane_val[i] = w;
        __syncthreads();
        double best = tol;
        int32_t enter = -1;
        for (uint32_t l = 0; l < L; ++l) {
            const double v = lane_val[l];
            if (!((P >> l) & 1ull) && v > best) {
                best = v;
                enter = (int32_t)l;
            }
        }
        enter = __builtin_amdgcn_readfirstlane(enter);
        __syncthreads();
        if (enter < 0) {
            status = 0;
            break;
        }
        P |= 1ull << enter;
        // 3. solve on P; step towards the solution until it is positive
        bool positive = false;
        while (n < cap) {
            n += 1u;
            const bool in = (P >> i) & 1ull;
            int32_t bad = 0;
            for (uint64_t mk = P; mk; mk &= mk - 1) {
                const uint32_t k = (uint32_t)__builtin_ctzll(mk);
                double s = 0.0;
                if (in && i >= k) {
                    s = A[i * S + k];
                    for (uint64_t m = P & ((1ull << k) - 1ull); m; m &= m - 1) {
                        const uint32_t mm = (uint32_t)__builtin_ctzll(m);
                        s = s - A[mm * S + i] * A[mm * S + k];
                    }
                    if (i == k)
                        piv = s;
                }
                __syncthreads();
                const double pk = piv;
                if (!(pk > 0.0 && pk < __builtin_huge_val())) {
                    bad = (int32_t)k + 1;
                    break;
                }
                const double d = sqrt(pk);
                if (i == k)
                    diag[k] = d;
                else if (in && i > k)
                    A[k * S + i] = s / d;
                __syncthreads();
            }
            if (bad) {
                if (row)
                    rgb[(size_t)rig * L * 3u + (size_t)i * 3u + c] = __builtin_nanf("");
                if (i == 0u) {
                    info[rig * 3u + c] = bad;
                    if (solves)
                        solves[rig * 3u + c] = (int32_t)n;
                }
                return;
            }
            double y = r;
            for (uint64_t mk = P; mk; mk &= mk - 1) {                // C z = r_P
                const uint32_t k = (uint32_t)__builtin_ctzll(mk);
                if (i == k)
                    sol[k] = y / diag[k];
                __syncthreads();
                if (in && i > k)
                    y = y - A[k * S + i] * sol[k];
            }
            if (in)
                y = sol[i];
            __syncthreads();
            for (uint64_t mk = P; mk;) {                             // C^T s = z, from the last column
                const uint32_t k = 63u - (uint32_t)__builtin_clzll(mk);
                mk &= ~(1ull << k);
                if (i == k)
                    sol[k] = y / diag[k];
                __syncthreads();
                if (in && i < k)
                    y = y - A[i * S + k] * sol[k];
            }
            const double s = in ? sol[i] : 0.0;
            const uint64_t blocked = __ballot(in && !(s > 0.0));
            if (blocked == 0ull) {
                if (in)
                    x = s;
                xs[i] = x;
                __syncthreads();
                positive = true;
                break;
            }
            lane_val[i] = x / (x - s);
            __syncthreads();
            uint32_t at = (uint32_t)__builtin_ctzll(blocked);
            double alpha = lane_val[at];
            for (uint64_t m = blocked & (blocked - 1); m; m &= m - 1) {
                const uint32_t l = (uint32_t)__builtin_ctzll(m);
                const double v = lane_val[l];
                if (v < alpha) {
                    alpha = v;
                    at = l;
                }
            }
            at = (uint32_t)__builtin_amdgcn_readfirstlane((int32_t)at);
            if (in) {
                const double step = s - x;
                const double move = alpha * step;
                x = x + move;
            }
            if (i == at)
                x = 0.0;
            const uint64_t leave = __ballot(in && !(x > 0.0));
            if ((leave >> i) & 1ull)
                x = 0.0;
            P &= ~leave;
            xs[i] = x;
            __syncthreads();
        }
        if (!positive)                                               // n == cap
            break;
    }
    if (row)
        rgb[(size_t)rig * L * 3u + (size_t)i * 3u + c] = (float)x;
    if (i == 0u) {
        info[rig * 3u + c] = status;
        if (solves)
            solves[rig * 3u + c] = (int32_t)n;
    }
}

template <int SLOTS>
void launch_partials(dim3 grid, hipStream_t stream, const float *final_shading, const float *albedo, const float *image, int nhwc,
                     const float *weight, int per_face, uint32_t L, uint32_t HW, uint32_t n_entries, double *partials)
{
    hipLaunchKernelGGL(light_fit_partials_kernel<SLOTS>, grid, dim3(kFitLanes), 0, stream, final_shading, albedo, image, nhwc, weight,
                       per_face, L, HW, n_entries, partials);
}

}  // namespace gcfr

using namespace gcfr;

extern "C" size_t gcfr_light_fit_workspace_bytes(int32_t B, int32_t L, int32_t H, int32_t W)
{
    if (!fit_shape_ok(B, L, H, W))
        return 0;
    return (size_t)B * fit_groups((uint32_t)B, (uint32_t)H * (uint32_t)W) * fit_entries((uint32_t)L) * sizeof(double);
}

extern "C" int gcfr_light_fit_normal(const float *final_shading, const float *albedo, const float *image, int32_t image_nhwc,
                                     const float *weight, int32_t weight_batch, int32_t B, int32_t L, int32_t H, int32_t W,
                                     void *workspace, double *gram, double *rhs, void *stream)
{
    if (!final_shading || !albedo || !image || !workspace || !gram || !rhs || !fit_shape_ok(B, L, H, W))
        return GCFR_ERR_INVALID_ARGUMENT;
    if ((image_nhwc != 0 && image_nhwc != 1) || (weight && weight_batch != 1 && weight_batch != B))
        return GCFR_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)workspace & 7u) || ((uintptr_t)gram & 7u) || ((uintptr_t)rhs & 7u))
        return GCFR_ERR_INVALID_ARGUMENT;
    const uint32_t HW = (uint32_t)H * (uint32_t)W, n = fit_entries((uint32_t)L), groups = fit_groups((uint32_t)B, HW);
    const int per_face = weight && weight_batch == B && B > 1 ? 1 : 0;
    double *partials = (double *)workspace;
    const dim3 grid(groups, (uint32_t)B);
    const hipStream_t s = (hipStream_t)stream;
    const uint32_t slots = (n + kFitLanes - 1) / kFitLanes;
#define GCFR_FIT_LAUNCH(S) launch_partials<S>(grid, s, final_shading, albedo, image, image_nhwc, weight, per_face, (uint32_t)L, HW, n, partials)
    if (slots <= 1)
        GCFR_FIT_LAUNCH(1);
    else if (slots <= 2)
        GCFR_FIT_LAUNCH(2);
    else if (slots <= 4)
        GCFR_FIT_LAUNCH(4);
    else if (slots <= 8)
        GCFR_FIT_LAUNCH(8);
    else if (slots <= 13)
        GCFR_FIT_LAUNCH(13);
    else if (slots <= 20)
        GCFR_FIT_LAUNCH(20);
    else
        GCFR_FIT_LAUNCH(26);
#undef GCFR_FIT_LAUNCH
    if (hipGetLastError() != hipSuccess)
        return GCFR_ERR_LAUNCH;
    hipLaunchKernelGGL(light_fit_finish_kernel, dim3((n + kFitLanes - 1) / kFitLanes, (uint32_t)B), dim3(kFitLanes), 0, s, partials,
                       groups, (uint32_t)L, n, gram, rhs);
    return hipGetLastError() == hipSuccess ? GCFR_OK : GCFR_ERR_LAUNCH;
}

extern "C" int gcfr_light_fit_solve(const double *gram, const double *rhs, int32_t B, int32_t L, double ridge, int32_t rgb_batch,
                                    float *rgb, int32_t *info, void *stream)
{
    if (!gram || !rhs || !rgb || !info || B < 1 || B > kFitMaxFaces || L < 1 || L > kFitMaxLights)
        return GCFR_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)gram & 7u) || ((uintptr_t)rhs & 7u) || (rgb_batch != 1 && rgb_batch != B))
        return GCFR_ERR_INVALID_ARGUMENT;
    if (!(ridge >= 0.0) || !std::isfinite(ridge))
        return GCFR_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(light_fit_solve_kernel, dim3(3u, (uint32_t)rgb_batch), dim3(kSolveLanes), 0, (hipStream_t)stream, gram, rhs,
                       (uint32_t)B, (uint32_t)L, ridge, (uint32_t)rgb_batch, rgb, info);
    return hipGetLastError() == hipSuccess ? GCFR_OK : GCFR_ERR_LAUNCH;
}

extern "C" int gcfr_light_fit_solve_nonneg(const double *gram, const double *rhs, int32_t B, int32_t L, double ridge, int32_t rgb_batch,
                                           int32_t max_solves, float *rgb, int32_t *info, int32_t *solves, void *stream)
{
    if (!gram || !rhs || !rgb || !info || B < 1 || B > kFitMaxFaces || L < 1 || L > kFitMaxLights)
        return GCFR_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)gram & 7u) || ((uintptr_t)rhs & 7u) || (rgb_batch != 1 && rgb_batch != B) || max_solves < 0)
        return GCFR_ERR_INVALID_ARGUMENT;
    if (!(ridge >= 0.0) || !std::isfinite(ridge))
        return GCFR_ERR_INVALID_ARGUMENT;
    const uint32_t cap = max_solves ? (uint32_t)max_solves : 3u * (uint32_t)L;
    hipLaunchKernelGGL(light_fit_solve_nonneg_kernel, dim3(3u, (uint32_t)rgb_batch), dim3(kSolveLanes), 0, (hipStream_t)stream, gram,
                       rhs, (uint32_t)B, (uint32_t)L, ridge, (uint32_t)rgb_batch, cap, rgb, info, solves);
    return hipGetLastError() == hipSuccess ? GCFR_OK : GCFR_ERR_LAUNCH;
}

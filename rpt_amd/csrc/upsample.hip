// upsample.hip — rpt_upsample*: the guided (joint-bilateral) upsampling of a low-resolution frame and its variance to s times the size
// on each axis, steered by the first-hit feature planes of both sizes (an addition: the reference renders every pixel it shows).  The
// arithmetic is the order of fp64 operations that include/rpt_hip.h states, every one rounded on its own (contraction off, IEEE
// division, no atomics): tests/upsample_ref.py restates it in numpy and the kernel's output is compared with it bit for bit.
//
// One kernel, one lane per full-resolution pixel, a plain grid of 32 x 8 pixel blocks (a wave = 32 x 2 neighbouring pixels, whose
// rows are 768 contiguous bytes of out_rgb).  A block's low-resolution footprint is (32 / s + 2 r) x (8 / s + 2 r) pixels, 18 x 6 at
// s = 2, r = 1: the (2 r)^2 taps of a lane are gathered from global memory, where the s^2 .. lanes that share a tap find it in L2.
// The kernel is instantiated per set of terms and flags (what is off costs no registers and no address arithmetic); s and r are
// arguments.
#include <hip/hip_runtime.h>

#include <utility>

#include "../../include/rpt_hip.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace rptg {
namespace {

constexpr uint32_t kTileX = 32, kTileY = 8;   // full-resolution pixels per block

// floor(t / d) for d > 0
__device__ __forceinline__ int64_t floor_div(int64_t t, int64_t d) {
    int64_t q = t / d;
    if (t - q * d < 0) q--;
    return q;
}

// One pixel, as include/rpt_hip.h orders it.  F: bit 0 the normal term, 1 the depth term, 2 DEMODULATE, 3 MATCH_ID.
template <uint32_t F>
__global__ __launch_bounds__(256) void upsample_kernel(const UpsampleArgs a) {
    constexpr bool NORMAL = F & 1u, DEPTH = F & 2u, DEMOD = F & 4u, MATCH = F & 8u;
    const uint32_t W = a.width * a.scale, H = a.height * a.scale;
    const uint32_t tiles_x = (W + kTileX - 1) / kTileX;
    const uint32_t by = blockIdx.x / tiles_x, bx = blockIdx.x - by * tiles_x;
    const uint32_t X = bx * kTileX + (threadIdx.x & (kTileX - 1)), Y = by * kTileY + threadIdx.x / kTileX;
    if (X >= W || Y >= H) return;
    const size_t p = size_t(Y) * W + X;
    const int64_t s = int64_t(a.scale), r = int64_t(a.radius);

    double den_p[3] = {1.0, 1.0, 1.0};
    if constexpr (DEMOD)
        for (int k = 0; k < 3; k++) {
            const double al = a.hi_albedo[3 * p + k];
            den_p[k] = al > 0.0 ? al : 1.0;   // (false for NaN)
        }
    double n_p[3] = {0.0, 0.0, 0.0}, z_p = 0.0, id_p = 0.0;
    if constexpr (NORMAL)
        for (int k = 0; k < 3; k++) n_p[k] = a.hi_normal[3 * p + k];
    if constexpr (DEPTH) z_p = a.hi_depth[3 * p];
    if constexpr (MATCH) id_p = a.hi_depth[3 * p + 2];

    const int64_t tx = 2 * int64_t(X) + 1 - s, ty = 2 * int64_t(Y) + 1 - s;
    const int64_t i0 = floor_div(tx, 2 * s), j0 = floor_div(ty, 2 * s);
    const double fx = double(tx - 2 * s * i0) / double(2 * s), fy = double(ty - 2 * s * j0) / double(2 * s);
    const double rd = double(r);

    // c and v of a low-resolution pixel
    auto lo_pixel = [&](size_t q, double c[3], double& v) {
        for (int k = 0; k < 3; k++) {
            double den = 1.0;
            if constexpr (DEMOD) {
                const double al = a.lo_albedo[3 * q + k];
                den = al > 0.0 ? al : 1.0;
            }
            c[k] = a.lo_rgb[3 * q + k] / den;
        }
        v = a.lo_var ? a.lo_var[q] : 0.0;
    };

    double Wsum = 0.0, C[3] = {0.0, 0.0, 0.0}, V = 0.0;
    for (int64_t dy = 1 - r; dy <= r; dy++) {
        const int64_t qy = j0 + dy;
        if (qy < 0 || qy >= int64_t(a.height)) continue;
        const double g_dy = 1.0 - fabs(fy - double(dy)) / rd;
        if (!(g_dy > 0.0)) continue;
        for (int64_t dx = 1 - r; dx <= r; dx++) {
            const int64_t qx = i0 + dx;
            if (qx < 0 || qx >= int64_t(a.width)) continue;
            const double g_dx = 1.0 - fabs(fx - double(dx)) / rd;
            if (!(g_dx > 0.0)) continue;
            const size_t q = size_t(qy) * a.width + size_t(qx);
            double x = 0.0;
            if constexpr (NORMAL) {
                const double e0 = (a.lo_normal[3 * q] - n_p[0]) * a.a_n, e1 = (a.lo_normal[3 * q + 1] - n_p[1]) * a.a_n,
                             e2 = (a.lo_normal[3 * q + 2] - n_p[2]) * a.a_n;
                x = x + ((e0 * e0 + e1 * e1) + e2 * e2);
            }
            if constexpr (DEPTH) {
                const double e = (a.lo_depth[3 * q] - z_p) * a.a_z;
                x = x + e * e;
            }
            bool ok = x < 4.0;                                        // (false for NaN)
            if constexpr (MATCH) ok = ok && a.lo_depth[3 * q + 2] == id_p;   // (false for NaN)
            if (!ok) continue;
            double c[3], v;
            lo_pixel(q, c, v);
            const double t = 1.0 - x * 0.25, t2 = t * t;
            const double wgt = (t2 * t2) * (g_dy * g_dx);
            Wsum = Wsum + wgt;
            C[0] = C[0] + wgt * c[0];
            C[1] = C[1] + wgt * c[1];
            C[2] = C[2] + wgt * c[2];
            V = V + (wgt * wgt) * v;
        }
    }
    double c[3], v;
    if (Wsum > 0.0) {
        c[0] = C[0] / Wsum;
        c[1] = C[1] / Wsum;
        c[2] = C[2] / Wsum;
        v = V / (Wsum * Wsum);
    } else {   // the pixel's own footprint
        lo_pixel(size_t(Y / a.scale) * a.width + X / a.scale, c, v);
    }
    a.out_rgb[3 * p] = c[0] * den_p[0];
    a.out_rgb[3 * p + 1] = c[1] * den_p[1];
    a.out_rgb[3 * p + 2] = c[2] * den_p[2];
    if (a.out_var) a.out_var[p] = v;
}

using UpsampleKernel = void (*)(const UpsampleArgs);
template <uint32_t... F>
constexpr UpsampleKernel kernel_of(uint32_t f, std::integer_sequence<uint32_t, F...>) {
    constexpr UpsampleKernel table[] = {upsample_kernel<F>...};
    return table[f];
}

}  // namespace

hipError_t launch_upsample(const UpsampleArgs& a, hipStream_t stream) {
    if (!a.width || !a.height) return hipSuccess;
    if (a.scale < 2 || a.scale > 4 || a.radius < 1 || a.radius > 2) return hipErrorInvalidValue;
    const uint64_t W = uint64_t(a.width) * a.scale, H = uint64_t(a.height) * a.scale;
    if (W * H >= (1ull << 31)) return hipErrorInvalidValue;
    const uint32_t f = (a.terms & 3u) | ((a.flags & RPT_UPSAMPLE_DEMODULATE) ? 4u : 0u) | ((a.flags & RPT_UPSAMPLE_MATCH_ID) ? 8u : 0u);
    // a plane the chosen instantiation reads must be there
    if (!a.lo_rgb || !a.out_rgb || ((f & 1u) && (!a.lo_normal || !a.hi_normal)) || ((f & 10u) && (!a.lo_depth || !a.hi_depth)) ||
        ((f & 4u) && (!a.lo_albedo || !a.hi_albedo)))
        return hipErrorInvalidValue;
    const uint32_t tiles = uint32_t((W + kTileX - 1) / kTileX) * uint32_t((H + kTileY - 1) / kTileY);
    hipLaunchKernelGGL(kernel_of(f, std::make_integer_sequence<uint32_t, 16>{}), dim3(tiles), dim3(kTileX * kTileY), 0, stream, a);
    return hipGetLastError();
}

}  // namespace rptg

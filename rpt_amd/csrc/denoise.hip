// denoise.hip — rpt_denoise*: the variance-guided edge-avoiding a-trous filter over a frame, its per-pixel variance and the
// first-hit feature planes (an addition: the reference has Filter::Box only).  The arithmetic is the order of fp64 operations that
// include/rpt_hip.h states, every one rounded on its own (contraction off, IEEE division, no atomics): tests/denoise_ref.py
// restates it in numpy and the kernels' output is compared with it bit for bit.
//
// Three kernels, plain grids of 16 x 16 pixel blocks (a wave = 16 x 4 neighbouring pixels):
//   denoise_prepare_kernel  demodulates and packs what a tap reads into one 64-byte record per pixel (c rgb, v, n xyz, z), the id
//                           beside it as a double; consecutive lanes write consecutive records.
//   denoise_pass_kernel     one lane per pixel and pass: vhat over the 3 x 3 neighbours, then the 5 x 5 taps at step s.  Two forms
//                           of the same device function: <false> gathers the records from global memory (L2), <true> stages the
//                           block's tile and its 2 s halo in LDS first ((16 + 4 s)^2 records of 72 bytes with the id: 28.8 KB at
//                           s = 1, 41.5 KB at s = 2; at s = 4 the tile would be four times the pixels it serves, and is not built).
//                           The last pass remodulates and writes the output planes in place of records.
//   buffer_mean_kernel / color_bytes_kernel   rpt_buffer_mean_device and the 8-bit image of rpt_buffer_denoised_image.
#include <hip/hip_runtime.h>

#include "../../include/rpt_hip.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace rptg {
namespace {

struct alignas(16) DenoiseRec {
    double c[3], v, n[3], z;
};
static_assert(sizeof(DenoiseRec) == 64, "one record is one 64-byte line");

constexpr uint32_t kTile = 16;         // pixels per block edge
constexpr uint32_t kLdsDoubles = 9;    // a staged record: the 8 doubles and the id (an odd stride in 8-byte words)

__global__ __launch_bounds__(256) void denoise_prepare_kernel(const DenoisePrepareArgs a) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= a.n_pixels) return;
    const size_t o = 3 * size_t(p);
    DenoiseRec r;
    for (int k = 0; k < 3; k++) {
        double den = 1.0;
        if (a.flags & RPT_DENOISE_DEMODULATE) {
            const double al = a.albedo[o + k];
            den = al > 0.0 ? al : 1.0;   // (false for NaN)
        }
        r.c[k] = a.rgb[o + k] / den;
        r.n[k] = a.normal ? a.normal[o + k] : 0.0;
    }
    r.v = a.var ? a.var[p] : 0.0;
    r.z = a.depth ? a.depth[o] : 0.0;
    reinterpret_cast<DenoiseRec*>(a.rec)[p] = r;
    a.ids[p] = a.depth ? a.depth[o + 2] : 0.0;
}

// Where a pass reads the records of its taps from.
struct GlobalSrc {
    const DenoiseRec* rec;
    const double* ids;
    uint32_t width;
    __device__ __forceinline__ size_t at(uint32_t x, uint32_t y) const { return size_t(y) * width + x; }
    __device__ __forceinline__ DenoiseRec load(uint32_t x, uint32_t y) const { return rec[at(x, y)]; }
    __device__ __forceinline__ double var(uint32_t x, uint32_t y) const { return rec[at(x, y)].v; }
    __device__ __forceinline__ double id(uint32_t x, uint32_t y) const { return ids[at(x, y)]; }
};
struct LdsSrc {
    const double* tile;      // [tw * tw][kLdsDoubles]
    uint32_t x0, y0, tw;     // image coordinates of the tile's first staged pixel + halo (may wrap below 0: only differences are used)
    __device__ __forceinline__ const double* at(uint32_t x, uint32_t y) const { return tile + size_t((y - y0) * tw + (x - x0)) * kLdsDoubles; }
    __device__ __forceinline__ DenoiseRec load(uint32_t x, uint32_t y) const {
        const double* q = at(x, y);
        DenoiseRec r;
        r.c[0] = q[0]; r.c[1] = q[1]; r.c[2] = q[2]; r.v = q[3];
        r.n[0] = q[4]; r.n[1] = q[5]; r.n[2] = q[6]; r.z = q[7];
        return r;
    }
    __device__ __forceinline__ double var(uint32_t x, uint32_t y) const { return at(x, y)[3]; }
    __device__ __forceinline__ double id(uint32_t x, uint32_t y) const { return at(x, y)[8]; }
};

// h = (1/16, 1/4, 3/8, 1/4, 1/16)
__device__ __forceinline__ double tap_weight(int d) { return d == 0 ? 0.375 : (d == 1 || d == -1 ? 0.25 : 0.0625); }
// One pixel of one pass, as include/rpt_hip.h orders it.
template <class Src>
__device__ __forceinline__ void denoise_pixel(const DenoisePassArgs& a, const Src& src, uint32_t x, uint32_t y) {
    const size_t p = size_t(y) * a.width + x;
    const DenoiseRec me = src.load(x, y);
    const double my_id = src.id(x, y);
    double den[3] = {1.0, 1.0, 1.0};
    if (a.flags & RPT_DENOISE_DEMODULATE)
        for (int k = 0; k < 3; k++) {
            const double al = a.albedo[3 * p + k];
            den[k] = al > 0.0 ? al : 1.0;
        }
    const bool color = a.terms & 1u, normal = a.terms & 2u, depth = a.terms & 4u, match = a.flags & RPT_DENOISE_MATCH_ID;
    double kp = 0.0;
    if (color) {
        double sv = 0.0, sg = 0.0;
#pragma unroll
        for (int dy = -1; dy <= 1; dy++)
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                const uint32_t qx = x + uint32_t(dx), qy = y + uint32_t(dy);   // (below 0 wraps to a large value)
                if (qx >= a.width || qy >= a.height) continue;
                const double gg = (dy == 0 ? 0.5 : 0.25) * (dx == 0 ? 0.5 : 0.25);
                sv = sv + gg * src.var(qx, qy);
                sg = sg + gg;
            }
        const double vhat = sv / sg;
        kp = 1.0 / (a.sigma_color2 * (vhat + 1e-12));
    }
    double W = 0.0, C[3] = {0.0, 0.0, 0.0}, V = 0.0;
    for (int dy = -2; dy <= 2; dy++) {
        const uint32_t qy = y + uint32_t(dy * int(a.step));
        if (qy >= a.height) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const uint32_t qx = x + uint32_t(dx * int(a.step));
            if (qx >= a.width) continue;
            const DenoiseRec q = src.load(qx, qy);
            double xx = 0.0;
            if (color) {
                const double e0 = (q.c[0] - me.c[0]) * den[0], e1 = (q.c[1] - me.c[1]) * den[1], e2 = (q.c[2] - me.c[2]) * den[2];
                xx = xx + ((e0 * e0 + e1 * e1) + e2 * e2) * kp;
            }
            if (normal) {
                const double e0 = (q.n[0] - me.n[0]) * a.a_n, e1 = (q.n[1] - me.n[1]) * a.a_n, e2 = (q.n[2] - me.n[2]) * a.a_n;
                xx = xx + ((e0 * e0 + e1 * e1) + e2 * e2);
            }
            if (depth) {
                const double e = (q.z - me.z) * a.a_z;
                xx = xx + e * e;
            }
            bool ok = xx < 4.0;                                  // (false for NaN)
            if (match) ok = ok && src.id(qx, qy) == my_id;       // (false for NaN)
            if (ok) {
                const double t = 1.0 - xx * 0.25, t2 = t * t;
                const double w = (t2 * t2) * (tap_weight(dy) * tap_weight(dx));
                W = W + w;
                C[0] = C[0] + w * q.c[0];
                C[1] = C[1] + w * q.c[1];
                C[2] = C[2] + w * q.c[2];
                V = V + (w * w) * q.v;
            }
        }
    }
    DenoiseRec out = me;
    if (W > 0.0) {
        out.c[0] = C[0] / W;
        out.c[1] = C[1] / W;
        out.c[2] = C[2] / W;
        out.v = V / (W * W);
    }
    if (a.out) {   // the last pass: remodulate
        a.out[3 * p] = out.c[0] * den[0];
        a.out[3 * p + 1] = out.c[1] * den[1];
        a.out[3 * p + 2] = out.c[2] * den[2];
        if (a.out_var) a.out_var[p] = out.v;
    } else {
        reinterpret_cast<DenoiseRec*>(a.rec_out)[p] = out;
    }
}

template <bool STAGED>
__global__ __launch_bounds__(256) void denoise_pass_kernel(const DenoisePassArgs a) {
    const uint32_t bx = blockIdx.x * kTile, by = blockIdx.y * kTile;
    const uint32_t x = bx + threadIdx.x, y = by + threadIdx.y;
    const DenoiseRec* const rec = reinterpret_cast<const DenoiseRec*>(a.rec_in);
    if constexpr (STAGED) {
        extern __shared__ double denoise_lds[];
        const uint32_t halo = 2u * a.step, tw = kTile + 2u * halo;
        const uint32_t x0 = bx - halo, y0 = by - halo;           // (may wrap: pixels left of / above the image fail the test below)
        for (uint32_t i = threadIdx.y * kTile + threadIdx.x; i < tw * tw; i += kTile * kTile) {
            const uint32_t ly = i / tw, lx = i - ly * tw;
            const uint32_t gx = x0 + lx, gy = y0 + ly;
            if (gx >= a.width || gy >= a.height) continue;       // never read: a tap outside the image is skipped
            const size_t g = size_t(gy) * a.width + gx;
            const DenoiseRec r = rec[g];
            double* const d = denoise_lds + size_t(i) * kLdsDoubles;
            d[0] = r.c[0]; d[1] = r.c[1]; d[2] = r.c[2]; d[3] = r.v;
            d[4] = r.n[0]; d[5] = r.n[1]; d[6] = r.n[2]; d[7] = r.z;
            d[8] = a.ids[g];
        }
        __syncthreads();
        if (x >= a.width || y >= a.height) return;
        denoise_pixel(a, LdsSrc{denoise_lds, x0, y0, tw}, x, y);
    } else {
        if (x >= a.width || y >= a.height) return;
        denoise_pixel(a, GlobalSrc{rec, a.ids, a.width}, x, y);
    }
}

// rpt_buffer_mean_device: sum / n in push order, and the variance of that mean.
__global__ __launch_bounds__(256) void buffer_mean_kernel(uint32_t n_pixels, uint32_t n_batches, const double* __restrict__ sum,
                                                          const double* __restrict__ sumsq, double* __restrict__ rgb, double* __restrict__ var) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n_pixels) return;
    const double n = double(n_batches);
    const double mr = sum[3 * size_t(p)] / n, mg = sum[3 * size_t(p) + 1] / n, mb = sum[3 * size_t(p) + 2] / n;
    rgb[3 * size_t(p)] = mr;
    rgb[3 * size_t(p) + 1] = mg;
    rgb[3 * size_t(p) + 2] = mb;
    if (var) {
        const double ss = sumsq[p] - n * ((mr * mr + mg * mg) + mb * mb);
        var[p] = fmax(ss, 0.0) / (n - 1.0) / n;
    }
}
// color_bytes (src/color.rs:18-24) of a frame, as buffer_image_kernel ends.
__global__ __launch_bounds__(256) void color_bytes_kernel(uint64_t n_values, const double* __restrict__ rgb, uint8_t* __restrict__ out) {
    const uint64_t i = uint64_t(blockIdx.x) * 256u + threadIdx.x;
    if (i >= n_values) return;
    const double v = fmin(fmax(rgb[i], 0.0), 1.0);               // NaN clamps to 0 like f64::clamp + `as u8`
    out[i] = uint8_t(pow(v, 1.0 / 2.2) * 255.0);
}

}  // namespace

hipError_t launch_denoise_prepare(const DenoisePrepareArgs& a, hipStream_t stream) {
    if (!a.n_pixels) return hipSuccess;
    hipLaunchKernelGGL(denoise_prepare_kernel, dim3((a.n_pixels + 255u) / 256u), dim3(256), 0, stream, a);
    return hipGetLastError();
}
hipError_t launch_denoise_pass(const DenoisePassArgs& a, bool staged, hipStream_t stream) {
    if (!a.width || !a.height) return hipSuccess;
    const dim3 grid((a.width + kTile - 1) / kTile, (a.height + kTile - 1) / kTile), block(kTile, kTile);
    if (staged) {
        if (a.step > kDenoiseMaxStagedStep) return hipErrorInvalidValue;
        const uint32_t tw = kTile + 4u * a.step;
        hipLaunchKernelGGL(denoise_pass_kernel<true>, grid, block, size_t(tw) * tw * kLdsDoubles * sizeof(double), stream, a);
    } else {
        hipLaunchKernelGGL(denoise_pass_kernel<false>, grid, block, 0, stream, a);
    }
    return hipGetLastError();
}
hipError_t launch_buffer_mean(uint32_t n_pixels, uint32_t n_batches, const double* d_sum, const double* d_sumsq, double* d_rgb, double* d_var,
                              hipStream_t st) {
    hipLaunchKernelGGL(buffer_mean_kernel, dim3((n_pixels + 255) / 256), dim3(256), 0, st, n_pixels, n_batches, d_sum, d_sumsq, d_rgb, d_var);
    return hipGetLastError();
}
hipError_t launch_color_bytes(uint64_t n_values, const double* d_rgb, uint8_t* d_out, hipStream_t st) {
    hipLaunchKernelGGL(color_bytes_kernel, dim3(uint32_t((n_values + 255) / 256)), dim3(256), 0, st, n_values, d_rgb, d_out);
    return hipGetLastError();
}

}  // namespace rptg

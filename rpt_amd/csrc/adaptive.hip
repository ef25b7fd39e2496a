// adaptive.hip — adaptive sampling by tile (an addition: the reference's Buffer keeps a Vec<Color> per pixel, src/buffer.rs:25-29,
// and its image() and variance() are defined for pixels with different sample counts, :59-93).  No render kernel is involved: a
// tile-list render hands the kernels of kernels.hip / kernels_f64.hip a caller's list of 32 x 32 tiles, and what is here is the
// buffer's side of it.
//   buffer_add_tiles_kernel         buffer_add_kernel's arithmetic on the in-image pixels of the listed tiles, and one more batch in
//                                   the per-tile counter of extra batches.
//   buffer_image_tiles_kernel, buffer_variance_tiles_kernel, buffer_mean_tiles_kernel
//                                   the read-outs of a buffer with extra batches: a pixel's count is n_batches + extra[its tile].
//   tile_errors_kernel              one block per tile: the per-pixel terms of include/rpt_hip.h, reduced by halving strides.
//   tile_select_kernel              one block: the ids of the tiles still above the threshold, ascending, and their number.
//   plane_tile_errors_kernel, tile_select_list_kernel
//                                   the same two over a tile list, the pixel's terms from planes (rpt_temporal_tile_errors_device and
//                                   the rounds of rpt_render_adaptive_temporal).
// The error and the mean are an order of fp64 operations, every one rounded on its own (contraction off, IEEE division, no
// atomics): tests/adaptive_ref.py restates them in numpy and the kernels' output is compared with it bit for bit.  The three
// kernels that repeat an expression of kernels.hip (add, image, variance) are compiled as that file is, so that a tile batch puts
// into a pixel the bits a full-frame batch would.
#include <hip/hip_runtime.h>

#include "../../include/rpt_hip.h"
#include "kernels.h"

namespace rptg {
namespace {

// Slot j of a tile in row-major order: pixel (32 tx + (j & 31), 32 ty + (j >> 5)).
__device__ __forceinline__ bool tile_slot_pixel(uint32_t tile, uint32_t j, uint32_t tiles_x, uint32_t width, uint32_t height, size_t& p) {
    const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const uint32_t x = tx * 32u + (j & 31u), y = ty * 32u + (j >> 5);
    p = size_t(y) * width + x;
    return x < width && y < height;
}
__device__ __forceinline__ uint32_t pixel_batches(const TileBufferView& b, uint32_t x, uint32_t y) {
    return b.n_batches + (b.extra ? b.extra[(y >> 5) * b.tiles_x + (x >> 5)] : 0u);
}

// ---- as kernels.hip compiles them
__global__ __launch_bounds__(256) void buffer_add_tiles_kernel(const TileBufferView b, const double* __restrict__ batch, double* __restrict__ sum,
                                                               double* __restrict__ sumsq, uint32_t* __restrict__ extra,
                                                               const uint32_t* __restrict__ tiles, uint32_t n_tiles) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;   // (n_tiles <= tiles_x * tiles_y < 2^21: no overflow)
    const uint32_t t = i >> 10, j = i & 1023u;
    if (t >= n_tiles) return;
    const uint32_t tile = tiles[t];
    if (tile >= b.tiles_x * b.tiles_y) return;            // an id from a list: checked before it indexes a per-tile array
    if (j == 0) extra[tile] += 1;                         // (distinct ids: one lane per counter)
    size_t p;
    if (!tile_slot_pixel(tile, j, b.tiles_x, b.width, b.height, p)) return;
    double r = batch[3 * p], g = batch[3 * p + 1], bl = batch[3 * p + 2];
    sum[3 * p] += r;
    sum[3 * p + 1] += g;
    sum[3 * p + 2] += bl;
    sumsq[p] += r * r + g * g + bl * bl;
}
// buffer_image_kernel with `count += samples[index].len()` (src/buffer.rs:85) per pixel of the window.
__global__ __launch_bounds__(256) void buffer_image_tiles_kernel(const TileBufferView b, uint32_t radius, const double* __restrict__ sum,
                                                                 uint8_t* __restrict__ out) {
    uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= b.width * b.height) return;
    uint32_t x = p % b.width, y = p / b.width;
    double r = 0.0, g = 0.0, bl = 0.0;
    uint64_t count = 0;
    uint32_t x0 = x >= radius ? x - radius : 0u, y0 = y >= radius ? y - radius : 0u;
    for (uint32_t i = x0; i <= x + radius; i++)
        for (uint32_t j = y0; j <= y + radius; j++)
            if (i < b.width && j < b.height) {
                size_t q = size_t(j) * b.width + i;
                r += sum[3 * q];
                g += sum[3 * q + 1];
                bl += sum[3 * q + 2];
                count += pixel_batches(b, i, j);
            }
    double c[3] = {r / double(count), g / double(count), bl / double(count)};
    for (int k = 0; k < 3; k++) {
        double v = fmin(fmax(c[k], 0.0), 1.0);               // NaN clamps to 0 like f64::clamp + `as u8`
        out[3 * size_t(p) + k] = uint8_t(pow(v, 1.0 / 2.2) * 255.0);
    }
}
__global__ __launch_bounds__(256) void buffer_variance_tiles_kernel(const TileBufferView b, const double* __restrict__ sum,
                                                                    const double* __restrict__ sumsq, double* __restrict__ out) {
    uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= b.width * b.height) return;
    double n = double(pixel_batches(b, p % b.width, p / b.width));
    double mr = sum[3 * size_t(p)] / n, mg = sum[3 * size_t(p) + 1] / n, mb = sum[3 * size_t(p) + 2] / n;
    double ss = sumsq[p] - n * (mr * mr + mg * mg + mb * mb);
    out[p] = fmax(ss, 0.0) / (n - 1.0);
}

// ---- the stated order of operations
#pragma clang fp contract(off)

// buffer_mean_kernel's m_k and v with n = double(n_p).
__device__ __forceinline__ void pixel_mean(const double* __restrict__ sum, const double* __restrict__ sumsq, size_t p, double n, double m[3],
                                           double& v) {
    m[0] = sum[3 * p] / n;
    m[1] = sum[3 * p + 1] / n;
    m[2] = sum[3 * p + 2] / n;
    const double ss = sumsq[p] - n * ((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
    v = fmax(ss, 0.0) / (n - 1.0) / n;
}
__global__ __launch_bounds__(256) void buffer_mean_tiles_kernel(const TileBufferView b, const double* __restrict__ sum,
                                                                const double* __restrict__ sumsq, double* __restrict__ rgb, double* __restrict__ var) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= b.width * b.height) return;
    double m[3], v;
    pixel_mean(sum, sumsq, p, double(pixel_batches(b, p % b.width, p / b.width)), m, v);
    rgb[3 * size_t(p)] = m[0];
    rgb[3 * size_t(p) + 1] = m[1];
    rgb[3 * size_t(p) + 2] = m[2];
    if (var) var[p] = v;
}

// One block per tile, lane l holds slots l, l + 256, l + 512, l + 768: strides 512 and 256 of the tree are the lane's own three
// additions, (a_l + a_{l+512}) + (a_{l+256} + a_{l+768}); strides 128 .. 1 run in LDS.
__global__ __launch_bounds__(256) void tile_errors_kernel(const TileBufferView b, double floor2, const double* __restrict__ sum,
                                                          const double* __restrict__ sumsq, double* __restrict__ err) {
    __shared__ double part[256];
    const uint32_t tile = blockIdx.x, l = threadIdx.x;       // (the grid is tiles_x * tiles_y blocks: every id is in range)
    const double n = double(b.n_batches + (b.extra ? b.extra[tile] : 0u));
    double a[4];
    for (uint32_t k = 0; k < 4; k++) {
        size_t p;
        a[k] = 0.0;
        if (!tile_slot_pixel(tile, l + 256u * k, b.tiles_x, b.width, b.height, p)) continue;
        double m[3], v;
        pixel_mean(sum, sumsq, p, n, m, v);
        const double y = (m[0] + m[1]) + m[2];
        a[k] = v / (y * y + floor2);
    }
    part[l] = (a[0] + a[2]) + (a[1] + a[3]);
    __syncthreads();
    for (uint32_t s = 128; s >= 1; s >>= 1) {
        if (l < s) part[l] = part[l] + part[l + s];
        __syncthreads();
    }
    if (l == 0) {
        const uint32_t ty = tile / b.tiles_x, tx = tile - ty * b.tiles_x;
        const uint32_t w = min(32u, b.width - tx * 32u), h = min(32u, b.height - ty * 32u);
        err[tile] = part[0] / double(w * h);
    }
}

// One block: flags of 256 tiles at a time, an inclusive scan of them in LDS, the running total carried from chunk to chunk.
__global__ __launch_bounds__(256) void tile_select_kernel(const TileBufferView b, double threshold2, uint32_t max_batches,
                                                          const double* __restrict__ err, uint32_t* __restrict__ out, uint32_t* __restrict__ n_out) {
    __shared__ uint32_t scan[256];
    const uint32_t l = threadIdx.x, n_tiles = b.tiles_x * b.tiles_y;
    uint32_t base = 0;
    for (uint32_t first = 0; first < n_tiles; first += 256u) {
        const uint32_t tile = first + l;
        uint32_t flag = 0;
        if (tile < n_tiles) {
            const uint32_t n_t = b.n_batches + (b.extra ? b.extra[tile] : 0u);
            flag = (err[tile] > threshold2 && n_t < max_batches) ? 1u : 0u;   // (false for a NaN error)
        }
        scan[l] = flag;
        __syncthreads();
        for (uint32_t s = 1; s < 256u; s <<= 1) {
            const uint32_t add = l >= s ? scan[l - s] : 0u;
            __syncthreads();
            scan[l] += add;
            __syncthreads();
        }
        if (flag) out[base + scan[l] - 1u] = tile;               // (base + scan <= tiles seen so far <= n_tiles: the list's capacity)
        base += scan[255];
        __syncthreads();
    }
    if (l == 0) *n_out = base;
}

// rpt_temporal_tile_errors_device: tile_errors_kernel's tree with the pixel's terms taken from planes, one block per listed tile
// (tiles null: block b is tile b).  On the planes buffer_mean(_tiles)_kernel wrote, y and v are the values tile_errors_kernel forms
// in registers, so the result is the same bits.
__global__ __launch_bounds__(256) void plane_tile_errors_kernel(uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t tiles_y, double floor2,
                                                                const double* __restrict__ rgb, const double* __restrict__ var,
                                                                const uint32_t* __restrict__ tiles, double* __restrict__ err) {
    __shared__ double part[256];
    const uint32_t tile = tiles ? tiles[blockIdx.x] : blockIdx.x, l = threadIdx.x;
    if (tile >= tiles_x * tiles_y) return;                    // an id from a list: checked before it indexes anything (the whole block leaves)
    double a[4];
    for (uint32_t k = 0; k < 4; k++) {
        size_t p;
        a[k] = 0.0;
        if (!tile_slot_pixel(tile, l + 256u * k, tiles_x, width, height, p)) continue;
        const double y = (rgb[3 * p] + rgb[3 * p + 1]) + rgb[3 * p + 2];
        a[k] = var[p] / (y * y + floor2);
    }
    part[l] = (a[0] + a[2]) + (a[1] + a[3]);
    __syncthreads();
    for (uint32_t s = 128; s >= 1; s >>= 1) {
        if (l < s) part[l] = part[l] + part[l + s];
        __syncthreads();
    }
    if (l == 0) {
        const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
        const uint32_t w = min(32u, width - tx * 32u), h = min(32u, height - ty * 32u);
        err[tile] = part[0] / double(w * h);
    }
}

// tile_select_kernel among a list (in null: among every tile): position i of `in` is flagged by its tile's error and count, the
// flagged ids keep their order.  `out` may be `in`: a chunk's ids are read before the chunk's barrier and written behind it, to
// positions <= their own, and no later chunk's position is written.
__global__ __launch_bounds__(256) void tile_select_list_kernel(const TileBufferView b, double threshold2, uint32_t max_batches,
                                                               const double* __restrict__ err, const uint32_t* in, uint32_t n_in,
                                                               uint32_t* out, uint32_t* __restrict__ n_out) {
    __shared__ uint32_t scan[256];
    const uint32_t l = threadIdx.x, n_tiles = b.tiles_x * b.tiles_y;
    const uint32_t n = in ? n_in : n_tiles;
    uint32_t base = 0;
    for (uint32_t first = 0; first < n; first += 256u) {
        const uint32_t i = first + l;
        uint32_t flag = 0, tile = 0;
        if (i < n) {
            tile = in ? in[i] : i;
            if (tile < n_tiles) {
                const uint32_t n_t = b.n_batches + (b.extra ? b.extra[tile] : 0u);
                flag = (err[tile] > threshold2 && n_t < max_batches) ? 1u : 0u;   // (false for a NaN error)
            }
        }
        scan[l] = flag;
        __syncthreads();
        for (uint32_t s = 1; s < 256u; s <<= 1) {
            const uint32_t add = l >= s ? scan[l - s] : 0u;
            __syncthreads();
            scan[l] += add;
            __syncthreads();
        }
        if (flag) out[base + scan[l] - 1u] = tile;               // (base + scan <= positions seen so far <= n: the list's capacity)
        base += scan[255];
        __syncthreads();
    }
    if (l == 0) *n_out = base;
}

}  // namespace

hipError_t launch_plane_tile_errors(uint32_t width, uint32_t height, double floor, const double* d_rgb, const double* d_var, const uint32_t* d_tiles,
                                    uint32_t n_tiles, double* d_err, hipStream_t st) {
    const uint32_t tiles_x = (width + 31u) / 32u, tiles_y = (height + 31u) / 32u;
    const uint32_t blocks = d_tiles ? n_tiles : tiles_x * tiles_y;
    if (!blocks) return hipSuccess;
    hipLaunchKernelGGL(plane_tile_errors_kernel, dim3(blocks), dim3(256), 0, st, width, height, tiles_x, tiles_y, floor * floor, d_rgb, d_var, d_tiles,
                       d_err);
    return hipGetLastError();
}
hipError_t launch_tile_select_list(const TileBufferView& b, double threshold2, uint32_t max_batches, const double* d_err, const uint32_t* d_tiles_in,
                                   uint32_t n_in, uint32_t* d_tiles_out, uint32_t* d_n_out, hipStream_t st) {
    hipLaunchKernelGGL(tile_select_list_kernel, dim3(1), dim3(256), 0, st, b, threshold2, max_batches, d_err, d_tiles_in, n_in, d_tiles_out, d_n_out);
    return hipGetLastError();
}

hipError_t launch_buffer_add_tiles(const TileBufferView& b, const double* d_batch, double* d_sum, double* d_sumsq, uint32_t* d_extra,
                                   const uint32_t* d_tiles, uint32_t n_tiles, hipStream_t st) {
    if (!n_tiles) return hipSuccess;
    hipLaunchKernelGGL(buffer_add_tiles_kernel, dim3(n_tiles * 4u), dim3(256), 0, st, b, d_batch, d_sum, d_sumsq, d_extra, d_tiles, n_tiles);
    return hipGetLastError();
}
hipError_t launch_buffer_image_tiles(const TileBufferView& b, uint32_t radius, const double* d_sum, uint8_t* d_out, hipStream_t st) {
    hipLaunchKernelGGL(buffer_image_tiles_kernel, dim3((b.width * b.height + 255) / 256), dim3(256), 0, st, b, radius, d_sum, d_out);
    return hipGetLastError();
}
hipError_t launch_buffer_variance_tiles(const TileBufferView& b, const double* d_sum, const double* d_sumsq, double* d_out, hipStream_t st) {
    hipLaunchKernelGGL(buffer_variance_tiles_kernel, dim3((b.width * b.height + 255) / 256), dim3(256), 0, st, b, d_sum, d_sumsq, d_out);
    return hipGetLastError();
}
hipError_t launch_buffer_mean_tiles(const TileBufferView& b, const double* d_sum, const double* d_sumsq, double* d_rgb, double* d_var,
                                    hipStream_t st) {
    hipLaunchKernelGGL(buffer_mean_tiles_kernel, dim3((b.width * b.height + 255) / 256), dim3(256), 0, st, b, d_sum, d_sumsq, d_rgb, d_var);
    return hipGetLastError();
}
hipError_t launch_tile_errors(const TileBufferView& b, double floor, const double* d_sum, const double* d_sumsq, double* d_err, hipStream_t st) {
    hipLaunchKernelGGL(tile_errors_kernel, dim3(b.tiles_x * b.tiles_y), dim3(256), 0, st, b, floor * floor, d_sum, d_sumsq, d_err);
    return hipGetLastError();
}
hipError_t launch_tile_select(const TileBufferView& b, double threshold2, uint32_t max_batches, const double* d_err, uint32_t* d_tiles_out,
                              uint32_t* d_n_out, hipStream_t st) {
    hipLaunchKernelGGL(tile_select_kernel, dim3(1), dim3(256), 0, st, b, threshold2, max_batches, d_err, d_tiles_out, d_n_out);
    return hipGetLastError();
}

}  // namespace rptg

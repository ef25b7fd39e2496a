// temporal.hip — rpt_temporal_*: temporal accumulation with reprojection for a camera moving over a scene whose objects keep their
// indices and either keep their places or move by a motion record per object (an addition: the reference renders every frame of a
// sequence from nothing).  The arithmetic is the order of fp64 operations that include/rpt_hip.h states, every one rounded on its
// own (contraction off, IEEE division and square root, no atomics): tests/temporal_ref.py and tests/temporal_motion_ref.py restate it
// in numpy and the kernel's output is compared with them bit for bit.
//
// One kernel, a plain grid of 16 x 16 pixel blocks (a wave = 16 x 4 neighbouring pixels), one lane per pixel: the pixel's surface point
// from the depth plane and the current camera record, its place in the previous frame from the stored record, up to four taps of the
// old history (one contiguous 80-byte record each; neighbouring lanes land on neighbouring records, so the taps of a wave overlap in
// L2), the blend, and the pixel's new record written to the other array.  Both camera records are kernel arguments, uniform over the
// grid.  A NULL plane is a uniform branch that yields the value the definition names (0.0), so the bits do not depend on it.
//
// RPT_TEMPORAL_CLIP is a third and fourth instantiation of the same kernel: before anything else the block stages the current frame's
// (16 + 2r)^2 halo -- the three colour planes and one "key" per cell that folds the count rule's inside-the-image, finite and id
// parts into one comparison -- in LDS; a pixel that took history then sums its window from LDS in the definition's order.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/rpt_hip.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace rptg {
namespace {

struct alignas(16) TemporalRec {
    double c[3], v, len, n[3], z, id;
};
static_assert(sizeof(TemporalRec) == kTemporalRecDoubles * sizeof(double), "one record is 80 contiguous bytes");

constexpr uint32_t kTile = 16;         // pixels per block edge
// The clip halo: at most (16 + 2 * 3)^2 cells of four doubles (r, g, b, key) as two arrays of rows of 48 doubles, r | b in columns
// 0..21 and g | key in columns 24..45.  A 32-lane half of a wave is two rows of 16 neighbouring pixels; it reads 16 consecutive
// doubles (32 banks of the 64 that an 8-byte LDS read sees) of two consecutive rows, and a pitch of 48 doubles = 96 dwords = 32
// (mod 64) puts the second row on the other 32 banks: no conflict at any radius or window offset.  (22, the smallest pitch, would
// overlap 12 banks: 2-way.)  16.5 KiB per block, nine blocks per CU.
constexpr uint32_t kHaloSide = kTile + 2 * kTemporalClipMaxRadius, kHaloPitch = 48, kHaloSecond = 24;
static_assert(kHaloSecond >= kHaloSide && kHaloSecond + kHaloSide <= kHaloPitch && (2 * kHaloPitch) % 64 == 32, "the halo's layout");

__device__ __forceinline__ double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ bool finite(double t) { return !(t - t != 0.0); }
// fmax and fmin as the clipping step defines them: the operand that is not NaN; of two that compare equal, the first
__device__ __forceinline__ double clip_max(double a, double b) { return (a >= b || b != b) ? a : b; }
__device__ __forceinline__ double clip_min(double a, double b) { return (a <= b || b != b) ? a : b; }

// MOTION: a table of motion records is set for the call (a.motion, a.n_motion): the pixel's point and normal go through the record
// of the pixel's object before the history is looked up.  Every lane loads its own record with plain vector loads: a wave is 16 x 4
// neighbouring pixels that nearly always see one or two ids, so the 21 loads of its lanes fall on the same few cache lines.
// CLIP: flag RPT_TEMPORAL_CLIP.  The key of a halo cell is NaN where the cell lies outside the image or its colour is not finite,
// else its id with MATCH_ID and 0.0 without; a cell counts iff key == (MATCH_ID ? the pixel's id : 0.0), which is false for NaN.
// PREVIEW: rpt_temporal_preview_device, steps 1 - 5 alone: the same kernel -- one body, so the two cannot differ by a bit -- whose
// argument carries a tile list and which writes no record.  With a list the grid is four blocks per listed 32 x 32 tile, block b the
// quadrant b & 3 (row-major) of tile tiles[b >> 2]; an id out of range and a quadrant outside the image are left by the whole block
// before anything else (no lane of it reaches the halo's barrier).  Without a list: the frame's ordinary grid.
struct TemporalPreviewArgs : TemporalArgs {
    const uint32_t* tiles;                               // [gridDim.x / 4] or null
    uint32_t tiles_x, tiles_y;
};
template <bool MOTION, bool CLIP, bool PREVIEW = false>
__global__ __launch_bounds__(256) void temporal_accumulate_kernel(const std::conditional_t<PREVIEW, TemporalPreviewArgs, TemporalArgs> a) {
    uint32_t bx = blockIdx.x, by = blockIdx.y;           // the block's place in the frame's grid of 16 x 16 pixel blocks
    if constexpr (PREVIEW) {
        if (a.tiles) {
            const uint32_t tile = a.tiles[blockIdx.x >> 2], q = blockIdx.x & 3u;
            if (tile >= a.tiles_x * a.tiles_y) return;
            const uint32_t ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
            bx = 2u * tx + (q & 1u);
            by = 2u * ty + (q >> 1);
            if (bx * kTile >= a.width || by * kTile >= a.height) return;
        }
    }
    const uint32_t x = bx * kTile + threadIdx.x, y = by * kTile + threadIdx.y;
    __shared__ double halo[CLIP ? 2 : 1][CLIP ? kHaloSide : 1][CLIP ? kHaloPitch : 1];
    if constexpr (CLIP) {
        // every thread of the block, the ones outside the image included, stages and reaches the barrier
        const uint32_t r = a.clip_radius, side = kTile + 2u * r;
        const bool match = a.flags & RPT_TEMPORAL_MATCH_ID;
        for (uint32_t i = threadIdx.y * kTile + threadIdx.x; i < side * side; i += kTile * kTile) {
            const uint32_t cy = i / side, cx = i - cy * side;
            const uint32_t gx = bx * kTile + cx - r, gy = by * kTile + cy - r;   // (left of / above the image wraps to a large value)
            double c0 = 0.0, c1 = 0.0, c2 = 0.0, key = __builtin_nan("");
            if (gx < a.width && gy < a.height) {
                const size_t g = size_t(gy) * a.width + gx;
                c0 = a.rgb[3 * g]; c1 = a.rgb[3 * g + 1]; c2 = a.rgb[3 * g + 2];
                if (finite(c0) && finite(c1) && finite(c2)) key = match ? a.depth[3 * g + 2] : 0.0;
            }
            halo[0][cy][cx] = c0;
            halo[0][cy][kHaloSecond + cx] = c1;
            halo[1][cy][cx] = c2;
            halo[1][cy][kHaloSecond + cx] = key;
        }
        __syncthreads();
    }
    if (x >= a.width || y >= a.height) return;
    const size_t p = size_t(y) * a.width + x;
    const double fw = double(a.width), fh = double(a.height), dim = double(a.width > a.height ? a.width : a.height);
    const double rgb[3] = {a.rgb[3 * p], a.rgb[3 * p + 1], a.rgb[3 * p + 2]};
    const double v_in = a.var ? a.var[p] : 0.0;
    // 2: the current surface point
    const double cov = a.depth[3 * p + 1];
    const bool hit = cov > 0.0;                                         // (false for NaN)
    const double zc = a.depth[3 * p] / cov, id = a.depth[3 * p + 2];
    double n[3] = {0.0, 0.0, 0.0};
    if (a.normal)
        for (int k = 0; k < 3; k++) n[k] = a.normal[3 * p + k];
    double B = 0.0, C[3] = {0.0, 0.0, 0.0}, V = 0.0, L = 0.0;
    if (a.have_history && hit) {
        // 1: the pixel centre's ray
        const double xn = (double(2u * x + 1u) - fw) / dim;
        const double yn = (double(2u * (a.height - y) - 1u) - fh) / dim;
        double v[3];
        for (int k = 0; k < 3; k++) v[k] = (a.cur.d * a.cur.dir[k] + xn * a.cur.right[k]) + yn * a.cur.up[k];
        const double l = __dsqrt_rn(dot3(v, v));
        // 3: where the history saw that point
        const double s = zc / l;
        double q[3];
        double nm[3] = {n[0], n[1], n[2]};                              // the normal the taps are tested against
        if constexpr (MOTION) {
            double P[3];
            for (int k = 0; k < 3; k++) P[k] = a.cur.eye[k] + s * v[k];
            if (id >= 1.0 && id <= double(a.n_motion)) {                // (false for NaN)
                const double* const r = a.motion + size_t(uint32_t(id) - 1u) * kTemporalMotionDoubles;
                const double P0 = P[0], P1 = P[1], P2 = P[2];
                for (int k = 0; k < 3; k++) {
                    P[k] = ((r[4 * k] * P0 + r[4 * k + 1] * P1) + r[4 * k + 2] * P2) + r[4 * k + 3];
                    nm[k] = (r[12 + 3 * k] * n[0] + r[13 + 3 * k] * n[1]) + r[14 + 3 * k] * n[2];
                }
            }
            for (int k = 0; k < 3; k++) q[k] = P[k] - a.prev.eye[k];
        } else {
            for (int k = 0; k < 3; k++) q[k] = (a.cur.eye[k] + s * v[k]) - a.prev.eye[k];
        }
        const double zq = dot3(q, a.prev.dir);
        if (zq > 0.0) {
            const double u = (dot3(q, a.prev.right) * a.prev.d) / zq;
            const double w = (dot3(q, a.prev.up) * a.prev.d) / zq;
            const double fx = ((u * dim + fw) - 1.0) * 0.5;
            const double fy = ((fh - 1.0) - w * dim) * 0.5;
            if (fx > -1.0 && fx < fw && fy > -1.0 && fy < fh) {          // (NaN fails)
                const double flx = floor(fx), fly = floor(fy);
                const double ax = fx - flx, ay = fy - fly;
                const int ix = int(flx), iy = int(fly);                   // -1 .. width - 1, -1 .. height - 1
                const double qq = dot3(q, q);
                const TemporalRec* const hist = reinterpret_cast<const TemporalRec*>(a.hist_in);
                const bool match = a.flags & RPT_TEMPORAL_MATCH_ID, depth = a.depth_tol > 0.0, normal = a.normal_tol > 0.0;
                const double nt2 = a.normal_tol * a.normal_tol;
#pragma unroll
                for (int j = 0; j < 2; j++)
#pragma unroll
                    for (int i = 0; i < 2; i++) {
                        const uint32_t tx = uint32_t(ix + i), ty = uint32_t(iy + j);   // (below 0 wraps to a large value)
                        if (tx >= a.width || ty >= a.height) continue;
                        const double b = (i ? ax : 1.0 - ax) * (j ? ay : 1.0 - ay);
                        const TemporalRec h = hist[size_t(ty) * a.width + tx];
                        bool ok = h.len > 0.0;                            // (every test: false for NaN)
                        if (match) ok = ok && h.id == id;
                        if (depth) {
                            const double r = h.z * h.z;
                            ok = ok && fabs(r - qq) <= a.depth_tol * qq;
                        }
                        if (normal) {
                            const double e0 = h.n[0] - nm[0], e1 = h.n[1] - nm[1], e2 = h.n[2] - nm[2];
                            ok = ok && ((e0 * e0 + e1 * e1) + e2 * e2) <= nt2;
                        }
                        if (ok) {
                            B = B + b;
                            C[0] = C[0] + b * h.c[0];
                            C[1] = C[1] + b * h.c[1];
                            C[2] = C[2] + b * h.c[2];
                            V = V + (b * b) * h.v;
                            L = L + b * h.len;
                        }
                    }
            }
        }
    }
    // 5: the blend
    TemporalRec out;
    double len = 1.0;
    if (B > 0.0) {
        const double hv = V / (B * B);
        double hl = L / B;
        double hc[3] = {C[0] / B, C[1] / B, C[2] / B};
        if constexpr (CLIP) {
            // between 4 and 5: the history colour clamped to the window of the current frame around the pixel itself
            const int r = int(a.clip_radius);
            const double want = (a.flags & RPT_TEMPORAL_MATCH_ID) ? id : 0.0;
            double n_w = 0.0, S[3] = {0.0, 0.0, 0.0}, Q[3] = {0.0, 0.0, 0.0};
            for (int dy = 0; dy <= 2 * r; dy++)
                for (int dx = 0; dx <= 2 * r; dx++) {
                    const uint32_t cy = threadIdx.y + dy, cx = threadIdx.x + dx;
                    if (halo[1][cy][kHaloSecond + cx] == want) {
                        const double c[3] = {halo[0][cy][cx], halo[0][cy][kHaloSecond + cx], halo[1][cy][cx]};
                        n_w = n_w + 1.0;
                        for (int k = 0; k < 3; k++) {
                            S[k] = S[k] + c[k];
                            Q[k] = Q[k] + c[k] * c[k];
                        }
                    }
                }
            if (n_w > 0.0) {
                bool clipped = false;
                for (int k = 0; k < 3; k++) {
                    const double m = S[k] / n_w;
                    const double s = clip_max(Q[k] / n_w - m * m, 0.0);
                    const double g = a.clip_gamma * __dsqrt_rn(s);
                    const double lo = m - g, hi = m + g;
                    const double t = clip_min(clip_max(hc[k], lo), hi);
                    clipped = clipped || t != hc[k];
                    hc[k] = t;
                }
                if (clipped && a.clip_history > 0u) hl = clip_min(hl, double(a.clip_history));
            }
        }
        len = fmin(hl + 1.0, double(a.max_history));
        const double al = 1.0 / len, om = 1.0 - al;
        for (int k = 0; k < 3; k++) out.c[k] = hc[k] + (rgb[k] - hc[k]) * al;
        out.v = (om * om) * hv + (al * al) * v_in;
    } else {
        out.c[0] = rgb[0]; out.c[1] = rgb[1]; out.c[2] = rgb[2];
        out.v = v_in;
    }
    a.out_rgb[3 * p] = out.c[0];
    a.out_rgb[3 * p + 1] = out.c[1];
    a.out_rgb[3 * p + 2] = out.c[2];
    if (a.out_var) a.out_var[p] = out.v;
    if (a.out_len) a.out_len[p] = len;
    if constexpr (PREVIEW) return;
    // 6: the new record; a miss or a value that is not finite carries no history
    const bool keep = hit && finite(out.c[0]) && finite(out.c[1]) && finite(out.c[2]) && finite(out.v);
    out.len = keep ? len : 0.0;
    out.n[0] = n[0]; out.n[1] = n[1]; out.n[2] = n[2];
    out.z = zc;
    out.id = id;
    reinterpret_cast<TemporalRec*>(a.hist_out)[p] = out;
}

}  // namespace

hipError_t launch_temporal_accumulate(const TemporalArgs& a, hipStream_t stream) {
    if (!a.width || !a.height) return hipSuccess;
    const dim3 grid((a.width + kTile - 1) / kTile, (a.height + kTile - 1) / kTile), block(kTile, kTile);
    if (a.flags & RPT_TEMPORAL_CLIP) {
        if (a.clip_radius < 1 || a.clip_radius > kTemporalClipMaxRadius) return hipErrorInvalidValue;   // the halo would not hold the window
        if (a.motion)
            hipLaunchKernelGGL((temporal_accumulate_kernel<true, true>), grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((temporal_accumulate_kernel<false, true>), grid, block, 0, stream, a);
    } else if (a.motion) {
        hipLaunchKernelGGL((temporal_accumulate_kernel<true, false>), grid, block, 0, stream, a);
    } else {
        hipLaunchKernelGGL((temporal_accumulate_kernel<false, false>), grid, block, 0, stream, a);
    }
    return hipGetLastError();
}

hipError_t launch_temporal_preview(const TemporalArgs& args, const uint32_t* d_tiles, uint32_t n_tiles, hipStream_t stream) {
    if (!args.width || !args.height || (d_tiles && !n_tiles)) return hipSuccess;
    TemporalPreviewArgs a{};
    static_cast<TemporalArgs&>(a) = args;
    a.tiles = d_tiles;
    a.tiles_x = (a.width + 31u) / 32u;
    a.tiles_y = (a.height + 31u) / 32u;
    if (d_tiles && n_tiles > a.tiles_x * a.tiles_y) return hipErrorInvalidValue;   // (distinct ids: a longer list cannot be; 4 n_tiles < 2^23)
    const dim3 grid = d_tiles ? dim3(4u * n_tiles) : dim3((a.width + kTile - 1) / kTile, (a.height + kTile - 1) / kTile), block(kTile, kTile);
    if (a.flags & RPT_TEMPORAL_CLIP) {
        if (a.clip_radius < 1 || a.clip_radius > kTemporalClipMaxRadius) return hipErrorInvalidValue;   // the halo would not hold the window
        if (a.motion)
            hipLaunchKernelGGL((temporal_accumulate_kernel<true, true, true>), grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((temporal_accumulate_kernel<false, true, true>), grid, block, 0, stream, a);
    } else if (a.motion) {
        hipLaunchKernelGGL((temporal_accumulate_kernel<true, false, true>), grid, block, 0, stream, a);
    } else {
        hipLaunchKernelGGL((temporal_accumulate_kernel<false, false, true>), grid, block, 0, stream, a);
    }
    return hipGetLastError();
}

hipError_t launch_temporal_motion_upload(void* d_table, const double* records, size_t bytes, hipStream_t stream) {
    return hipMemcpyAsync(d_table, records, bytes, hipMemcpyHostToDevice, stream);
}

}  // namespace rptg

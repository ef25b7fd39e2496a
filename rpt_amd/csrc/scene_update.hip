// scene_update.hip — the kernels of rpt_scene_move_spheres_device (include/rpt_hip.h, "moving spheres"; host half: rpt_scene_update.cpp).
//
//   move_spheres_kernel   a lane per movable sphere: the records of scene_update_core.h for its new centre, into the committed arenas
//   cull32_kernel         reference-epsilon mode: a wave per group of 32 records that holds a movable sphere, min / max by shuffles
//   refit_kernel          scene tree: the boxes of its nodes bottom-up, a lane per node of one height
//
// Every store is a plain vector store into a record no other lane of the launch writes; there is no atomic, no spin wait and no
// grid-wide synchronisation, and every loop's trip count is fixed by the arguments.  The render kernels read these arrays through the
// scalar cache and the vector L1: what is written here reaches them across a kernel boundary on one stream (the end of a kernel
// releases its stores, the start of the next one invalidates both caches), never inside a launch.
#include <hip/hip_runtime.h>

#include "scene_update_lanes.h"

namespace rptg {
namespace {
// (scene_update_core.h turns fp contraction off for the rest of this file: the padding of a node box relies on it too.)

__global__ __launch_bounds__(64) void move_spheres_kernel(SceneUpdateArgs a) {
    const uint32_t k = blockIdx.x * 64u + threadIdx.x;
    if (k < a.n) move_sphere_lane(a, k);
}

// The union box of records 32 g .. 32 g + 31 as the commit forms it (rpt_capi.cpp, build_scene64): min / max in record order, where
// the earlier record keeps a tie -- the butterfly below combines the lower half's value with the upper half's in that order at every
// step, which is the serial result --, `unbounded` if one of them is (its box then zero), slab_test = 2 if one of them is a cube.
__global__ __launch_bounds__(64) void cull32_kernel(SceneUpdateArgs a) {
    const uint32_t g = a.groups[blockIdx.x], lane = threadIdx.x;
    const uint32_t i = 32u * g + lane;
    const bool have = lane < 32u && i < a.n_objects;
    float lo[3] = {HUGE_VALF, HUGE_VALF, HUGE_VALF}, hi[3] = {-HUGE_VALF, -HUGE_VALF, -HUGE_VALF};
    uint32_t unbounded = 0u, slab = 0u;
    if (have) {
        const rpt64::CullBox cb = a.cull[i];
        for (int k = 0; k < 3; k++) { lo[k] = cb.lo[k]; hi[k] = cb.hi[k]; }
        unbounded = cb.unbounded ? 1u : 0u;
        slab = cb.slab_test ? 1u : 0u;
    }
    // lanes 32..63 hold the identity and exchange among themselves only (the steps stay below 32)
    for (int step = 1; step < 32; step <<= 1) {
        const bool upper = (lane & uint32_t(step)) != 0u;
        for (int k = 0; k < 3; k++) {
            const float ol = __shfl_xor(lo[k], step, 64), oh = __shfl_xor(hi[k], step, 64);
            lo[k] = upper ? rptu::min_std(ol, lo[k]) : rptu::min_std(lo[k], ol);
            hi[k] = upper ? rptu::max_std(oh, hi[k]) : rptu::max_std(hi[k], oh);
        }
        unbounded |= uint32_t(__shfl_xor(int(unbounded), step, 64));
        slab |= uint32_t(__shfl_xor(int(slab), step, 64));
    }
    if (lane == 0u) {
        rpt64::CullBox u;
        for (int k = 0; k < 3; k++) { u.lo[k] = unbounded ? 0.f : lo[k]; u.hi[k] = unbounded ? 0.f : hi[k]; }
        u.unbounded = unbounded;
        u.slab_test = slab ? 2u : 0u;
        a.cull32[g] = u;
    }
}

// Heights [h0, h1) of the scene tree; a lane per node of a height.  More than one height only with a grid of ONE workgroup: the
// barrier between two heights is the workgroup's, and its release / acquire at workgroup scope is what makes the bounds written for
// the height below visible to the lanes of this one (a workgroup runs on one compute unit).
__global__ __launch_bounds__(1024) void refit_kernel(SceneUpdateArgs a, uint32_t h0, uint32_t h1) {
    for (uint32_t h = h0; h < h1; h++) {
        const uint32_t first = a.height_first[h], last = a.height_first[h + 1];
        for (uint32_t i = first + blockIdx.x * blockDim.x + threadIdx.x; i < last; i += gridDim.x * blockDim.x) {
            const uint32_t node = a.order[i];
            refit_entry(a, node, 0u);
            refit_entry(a, node, 1u);
        }
        if (h + 1 < h1) __syncthreads();
    }
}
}  // namespace

hipError_t launch_scene_update_spheres(const SceneUpdateArgs& a, hipStream_t stream) {
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(move_spheres_kernel, dim3((a.n + 63u) / 64u), dim3(64), 0, stream, a);
    return hipGetLastError();
}
hipError_t launch_scene_update_cull32(const SceneUpdateArgs& a, hipStream_t stream) {
    if (a.n_groups == 0) return hipSuccess;
    hipLaunchKernelGGL(cull32_kernel, dim3(a.n_groups), dim3(64), 0, stream, a);
    return hipGetLastError();
}
hipError_t launch_scene_update_refit(const SceneUpdateArgs& a, bool per_height, hipStream_t stream) {
    if (a.n_tree == 0 || a.n_heights == 0) return hipSuccess;
    if (!per_height) {
        hipLaunchKernelGGL(refit_kernel, dim3(1), dim3(1024), 0, stream, a, 0u, a.n_heights);
        return hipGetLastError();
    }
    for (uint32_t h = 0; h < a.n_heights; h++) {
        const uint32_t n = a.height_first[h + 1] - a.height_first[h];
        if (n == 0) continue;
        hipLaunchKernelGGL(refit_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, a, h, h + 1u);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
}  // namespace rptg

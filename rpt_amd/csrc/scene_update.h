// scene_update.h — what rpt_scene_update.cpp hands to scene_update.hip: the tables rpt_scene_set_movable_spheres uploads and the
// launchers of rpt_scene_move_spheres_device (weak, as in particles.h: a host build without the kernels links, and the entry points then
// report RPT_ERR_UNSUPPORTED; the CPU harness defines them over scene_update_core.h).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "f64_layout.h"
#include "gpu_layout.h"

namespace rptg {
// One movable sphere (48 bytes).  `centre` is the state: the kernel reads the previous centre from it and writes the new one.
struct MovableSphere {
    uint32_t sph;       // index of its record in SceneView::sph / sph_sh / pbox (spheres come first in pbox)
    uint32_t object;    // index into scene.objects = its row of the motion table
    uint32_t rec64;     // reference-epsilon mode: index into Scene::recs / shade / cull
    uint32_t reserved;
    double radius;
    double centre[3];
};
// One child entry of a scene-tree node, 2 i + side for local node i (32 bytes): how the refit forms its box.
//   a == kRefitInner: the union of the two entries of local node b;
//   else: the fixed box (the entry's items that cannot move; lo = +inf, hi = -inf if there are none) united with the item boxes of
//   movable spheres a and b (kRefitNone: no sphere).  An entry that is the root of a mesh tree is all fixed box.
struct RefitEntry {
    float lo[3];
    uint32_t a;
    float hi[3];
    uint32_t b;
};
static constexpr uint32_t kRefitNone = 0xFFFFFFFFu, kRefitInner = 0xFFFFFFFEu;
static constexpr uint32_t kRefitMaxHeights = 32;   // the walk's stack bounds the tree's depth (rpt_scene_commit)
struct SceneUpdateArgs {
    MovableSphere* table;
    uint32_t n;                 // movable spheres
    uint32_t f64;               // 1: the scene was committed in the reference-epsilon mode (recs, shade, cull are written as well)
    const double* centres;      // [n * 3]
    const double* offsets;      // [n * 3] or null
    double* motion;             // [n_obj * 24] or null: rows of the listed objects are written
    // fp32 arena
    XfScan* sph;
    XfShade* sph_sh;
    AabbScan* pbox;
    float* item_box;            // [n * 8]: xf_box of every movable sphere (lo, -, hi, -), what the refit reads
    // reference-epsilon arena
    rpt64::ObjRec* recs;
    rpt64::ObjShade* shade;
    rpt64::CullBox* cull;
    rpt64::CullBox* cull32;
    const uint32_t* groups;     // the cull32 groups that hold a movable sphere
    uint32_t n_groups, n_objects;
    // scene tree (scene_bvh = 1): local node i is nodes[top_root + i]
    BvhNode* nodes;
    uint32_t top_root, n_tree;  // n_tree: nodes of the scene tree (0: none)
    const RefitEntry* entries;  // [2 * n_tree]
    float* raw;                 // [2 * n_tree * 8]: the unpadded bounds of every entry (lo, -, hi, -)
    const uint32_t* order;      // [n_tree]: local nodes by height, children before parents
    uint32_t n_heights;
    uint32_t height_first[kRefitMaxHeights + 1];   // order[height_first[h] .. height_first[h + 1]): the nodes of height h
};
// The records of the moved spheres, their centres and motion rows: one lane per sphere.
__attribute__((weak)) hipError_t launch_scene_update_spheres(const SceneUpdateArgs& a, hipStream_t stream);
// cull32 of the groups in a.groups: one wave per group.
__attribute__((weak)) hipError_t launch_scene_update_cull32(const SceneUpdateArgs& a, hipStream_t stream);
// The scene tree's boxes, bottom-up.  per_height = false: one workgroup walks heights [0, n_heights) with a barrier between two;
// true: one launch per height.
__attribute__((weak)) hipError_t launch_scene_update_refit(const SceneUpdateArgs& a, bool per_height, hipStream_t stream);
}  // namespace rptg

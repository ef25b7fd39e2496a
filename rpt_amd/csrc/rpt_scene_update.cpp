// rpt_scene_update.cpp — host half of "moving spheres" (include/rpt_hip.h): rpt_sphere_records_host, rpt_scene_set_movable_spheres,
// rpt_scene_move_spheres*, rpt_scene_movable_info and rpt_debug_scene_records.  Pure host code over the committed scene of
// scene_host.h; the kernels are scene_update.hip's, the arithmetic of a record is scene_update_core.h's.
// tests/host/scene_update_harness.cpp runs all of it with malloc-backed HIP stubs.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/rpt_hip.h"
#include "scene_host.h"
#include "scene_update.h"
#include "scene_update_core.h"

using rpti::fail;
using namespace rptg;

namespace {
uint32_t count_spheres(const HShape& h) {   // sphere records the flattener's emit makes of a shape
    if (h.d.kind == RPT_SHAPE_SPHERE) return 1;
    uint32_t n = 0;
    for (const HShape& c : h.children) n += count_spheres(c);
    return n;
}
uint32_t count_leaves(const HShape& h) {    // records the fp64 flatten makes of a shape
    if (h.d.kind != RPT_SHAPE_GROUP) return 1;
    uint32_t n = 0;
    for (const HShape& c : h.children) n += count_leaves(c);
    return n;
}
std::string obj_name(uint32_t o) { return "object " + std::to_string(o); }

// What the list must satisfy, object by object in list order (include/rpt_hip.h states the order); radius and centre of each.
int check_movable(const rpt_scene* s, const uint32_t* objects, uint32_t n, std::vector<double>& radius, std::vector<double>& centre) {
    std::vector<bool> seen(s->objects.size(), false);
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t o = objects[k];
        if (o >= s->objects.size()) return fail(RPT_ERR_INVALID, "movable spheres: entry " + std::to_string(k) + " names " + obj_name(o) + ", the scene has " + std::to_string(s->objects.size()));
        if (seen[o]) return fail(RPT_ERR_INVALID, "movable spheres: " + obj_name(o) + " is listed twice");
        seen[o] = true;
        const rpt_shape_desc& d = s->objects[o].shape.d;
        if (d.kind == RPT_SHAPE_GROUP) return fail(RPT_ERR_UNSUPPORTED, "movable spheres: " + obj_name(o) + " is a group (its members cannot move)");
        if (d.kind != RPT_SHAPE_SPHERE) return fail(RPT_ERR_INVALID, "movable spheres: " + obj_name(o) + " is not a sphere");
        for (const rptg::Light& L : s->light_records)
            if (L.kind == L_OBJECT && L.twin_object == int32_t(o))
                return fail(RPT_ERR_UNSUPPORTED, "movable spheres: " + obj_name(o) + " is the twin of a Light::Object (the light's sampler would stay behind)");
        if (!d.has_transform) return fail(RPT_ERR_INVALID, "movable spheres: " + obj_name(o) + " has no transform (translate(c) * scale(r, r, r) is required)");
        const double* M = d.transform;
        const double r = M[0];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++)
                if (i != j && M[4 * i + j] != 0.0) return fail(RPT_ERR_INVALID, "movable spheres: the transform of " + obj_name(o) + " has a non-zero off-diagonal (rotation or shear)");
        if (M[5] != r || M[10] != r) return fail(RPT_ERR_INVALID, "movable spheres: the transform of " + obj_name(o) + " does not scale uniformly");
        if (!std::isfinite(r) || !(r > 0.0)) return fail(RPT_ERR_INVALID, "movable spheres: the radius of " + obj_name(o) + " must be finite and > 0");
        if (M[12] != 0.0 || M[13] != 0.0 || M[14] != 0.0 || M[15] != 1.0) return fail(RPT_ERR_INVALID, "movable spheres: the bottom row of the transform of " + obj_name(o) + " must be 0 0 0 1");
        for (int i = 0; i < 3; i++)
            if (!std::isfinite(M[4 * i + 3])) return fail(RPT_ERR_INVALID, "movable spheres: the centre of " + obj_name(o) + " is not finite");
        // the radius must admit a motion record: det and det' of a move to the origin (they depend on r alone)
        const double from[3] = {1.0, 1.0, 1.0}, origin[3] = {0.0, 0.0, 0.0};
        double rec[24];
        if (!rptu::sphere_motion_record(r, origin, from, rec))
            return fail(RPT_ERR_INVALID, "movable spheres: the radius of " + obj_name(o) + " admits no motion record (its determinant is zero or not finite)");
        radius.push_back(r);
        const auto moved = s->dev.moved_centres.find(o);   // (a sphere an earlier list has moved is where that list left it)
        for (int i = 0; i < 3; i++) centre.push_back(moved != s->dev.moved_centres.end() ? moved->second[size_t(i)] : M[4 * i + 3]);
    }
    return RPT_OK;
}

void fill_args(rpt_scene* s, SceneUpdateArgs& a) {
    auto& m = s->dev.mov;
    std::memset(&a, 0, sizeof(a));
    a.table = m.d_table.get<MovableSphere>();
    a.n = m.n;
    a.f64 = s->dev.arena64 ? 1u : 0u;
    a.sph = const_cast<XfScan*>(s->view.sph);
    a.sph_sh = const_cast<XfShade*>(s->view.sph_sh);
    a.pbox = const_cast<AabbScan*>(s->view.pbox);
    a.item_box = m.d_item_box.get<float>();
    if (a.f64) {
        a.recs = const_cast<rpt64::ObjRec*>(s->view64.recs);
        a.shade = const_cast<rpt64::ObjShade*>(s->view64.shade);
        a.cull = const_cast<rpt64::CullBox*>(s->view64.cull);
        a.cull32 = const_cast<rpt64::CullBox*>(s->view64.cull32);
        a.groups = m.d_groups.get<uint32_t>();
        a.n_groups = m.n_groups;
        a.n_objects = s->view64.n_objects;
    }
    a.nodes = const_cast<BvhNode*>(s->view.nodes);
    a.top_root = s->view.top_root;
    a.n_tree = m.n_tree;
    a.entries = m.d_entries.get<RefitEntry>();
    a.raw = m.d_raw.get<float>();
    a.order = m.d_order.get<uint32_t>();
    a.n_heights = m.n_heights;
    for (size_t h = 0; h < m.height_first.size(); h++) a.height_first[h] = m.height_first[h];
}
}  // namespace

extern "C" {

int rpt_sphere_records_host(double radius, const double centre[3], const double prev_centre[3], float scan[12], float shade[12],
                            float item_box[6], float pbox[8], double inv[12], double nrm[9], void* cull, double motion[24]) {
    if (!centre) return fail(RPT_ERR_INVALID, "null centre");
    rptu::SphereRecords r;
    rptu::sphere_records(radius, centre, &r);
    if (scan) std::memcpy(scan, r.scan, sizeof(r.scan));
    if (shade) {
        const float one = 1.f;
        for (int i = 0; i < 12; i++) shade[i] = 0.f;
        shade[0] = shade[5] = shade[10] = r.shade_n;
        shade[7] = one;   // r1.w: the shape is wrapped in Transformed (r0.w, the object id, is the caller's)
    }
    if (item_box)
        for (int i = 0; i < 3; i++) { item_box[i] = r.item_lo[i]; item_box[3 + i] = r.item_hi[i]; }
    if (pbox)
        for (int i = 0; i < 4; i++) { pbox[i] = i < 3 ? r.pbox_lo[i] : 0.f; pbox[4 + i] = i < 3 ? r.pbox_hi[i] : 0.f; }
    if (inv) std::memcpy(inv, r.inv, sizeof(r.inv));
    if (nrm)
        for (int i = 0; i < 9; i++) nrm[i] = (i == 0 || i == 4 || i == 8) ? r.nrm : 0.0;
    if (cull) {
        rpt64::CullBox cb{};
        for (int i = 0; i < 3; i++) { cb.lo[i] = r.cull_lo[i]; cb.hi[i] = r.cull_hi[i]; }
        cb.unbounded = r.cull_unbounded;
        std::memcpy(cull, &cb, sizeof(cb));
    }
    if (motion) {
        if (!prev_centre) return fail(RPT_ERR_INVALID, "a motion record needs the previous centre");
        if (!rptu::sphere_motion_record(radius, centre, prev_centre, motion))
            return fail(RPT_ERR_INVALID, "motion record: rpt_temporal_motion_record refuses these matrices (a value is not finite, or a determinant is zero)");
    }
    return RPT_OK;
}

int rpt_scene_set_movable_spheres(rpt_scene* s, const uint32_t* objects, uint32_t n) {
    if (!s) return fail(RPT_ERR_INVALID, "null scene");
    if (!objects && n) return fail(RPT_ERR_INVALID, "null object list");
    if (!s->committed) return fail(RPT_ERR_STATE, "rpt_scene_commit must be called before rpt_scene_set_movable_spheres");
    std::vector<double> radius, centre;
    if (int rc = check_movable(s, objects, n, radius, centre)) return rc;
    if (!launch_scene_update_spheres || !launch_scene_update_cull32 || !launch_scene_update_refit)
        return fail(RPT_ERR_UNSUPPORTED, "rpt_scene_set_movable_spheres: built without the kernels");
    RPTI_HIP_TRY(hipSetDevice(s->device));
    auto& old = s->dev.mov;
    if (old.used) RPTI_HIP_TRY(hipEventSynchronize(old.done.get()));   // (its tables are freed below)
    if (old.set && old.n && old.moves) {   // where the spheres of the list being replaced are now: the state lives in the device table
        std::vector<MovableSphere> was(old.n);
        RPTI_HIP_TRY(hipMemcpy(was.data(), old.d_table.get(), was.size() * sizeof(MovableSphere), hipMemcpyDeviceToHost));
        for (const MovableSphere& m : was) s->dev.moved_centres[m.object] = {m.centre[0], m.centre[1], m.centre[2]};
        for (uint32_t k = 0; k < n; k++)
            for (int i = 0; i < 3; i++) {
                const auto it = s->dev.moved_centres.find(objects[k]);
                if (it != s->dev.moved_centres.end()) centre[3 * size_t(k) + size_t(i)] = it->second[size_t(i)];
            }
    }

    const bool f64 = bool(s->dev.arena64);
    // where each listed object's records are: spheres in emit order, fp64 records in flatten order
    std::vector<uint32_t> sph_before(s->objects.size() + 1, 0), rec_before(s->objects.size() + 1, 0);
    for (size_t o = 0; o < s->objects.size(); o++) {
        sph_before[o + 1] = sph_before[o] + count_spheres(s->objects[o].shape);
        rec_before[o + 1] = rec_before[o] + count_leaves(s->objects[o].shape);
    }
    if (sph_before.back() != s->view.n_sph || (f64 && rec_before.back() != s->view64.n_objects))
        return fail(RPT_ERR_STATE, "movable spheres: the committed record counts are not the scene's");
    std::unordered_map<uint32_t, uint32_t> object_of_sph;   // top-level spheres only: the ones a list can have moved
    for (size_t o = 0; o < s->objects.size(); o++)
        if (s->objects[o].shape.d.kind == RPT_SHAPE_SPHERE) object_of_sph[sph_before[o]] = uint32_t(o);
    std::vector<MovableSphere> table(n);
    std::vector<float> item_box(size_t(n) * 8, 0.f);
    std::unordered_map<uint32_t, uint32_t> slot_of_sph;
    for (uint32_t k = 0; k < n; k++) {
        MovableSphere& m = table[k];
        m.sph = sph_before[objects[k]];
        m.object = objects[k];
        m.rec64 = rec_before[objects[k]];
        m.reserved = 0;
        m.radius = radius[k];
        for (int i = 0; i < 3; i++) m.centre[i] = centre[3 * k + i];
        rptu::sphere_item_box(m.radius, m.centre, &item_box[8 * size_t(k)], &item_box[8 * size_t(k) + 4]);
        slot_of_sph[m.sph] = k;
    }
    // reference-epsilon mode: the cull32 groups to recompute
    std::vector<uint32_t> groups;
    if (f64) {
        for (const MovableSphere& m : table) groups.push_back(m.rec64 / 32u);
        std::sort(groups.begin(), groups.end());
        groups.erase(std::unique(groups.begin(), groups.end()), groups.end());
    }
    // scene tree: per child entry how the refit forms its box, and the nodes by height
    std::vector<RefitEntry> entries;
    std::vector<float> raw;
    std::vector<uint32_t> order, height_first;
    uint32_t n_tree = 0, n_heights = 0;
    if (s->view.scene_bvh && n != 0) {
        n_tree = s->view.n_nodes - s->view.top_root;
        const size_t n_pleaf = size_t(s->stats[11]);
        if (s->tree_raw.size() != size_t(n_tree) * 12 || s->pleaf_box.size() != n_pleaf * 6)
            return fail(RPT_ERR_STATE, "movable spheres: the commit's record of the scene tree does not match the tree");
        std::vector<BvhNode> nodes(n_tree);
        std::vector<uint32_t> pleaf(n_pleaf);
        if (n_tree) RPTI_HIP_TRY(hipMemcpy(nodes.data(), s->view.nodes + s->view.top_root, size_t(n_tree) * sizeof(BvhNode), hipMemcpyDeviceToHost));
        if (n_pleaf) RPTI_HIP_TRY(hipMemcpy(pleaf.data(), s->view.pleaf, n_pleaf * 4, hipMemcpyDeviceToHost));
        entries.resize(size_t(n_tree) * 2);
        raw.assign(size_t(n_tree) * 16, 0.f);
        std::vector<uint32_t> height(n_tree, 0);
        const float inf = std::numeric_limits<float>::infinity();
        for (uint32_t i = n_tree; i-- > 0;) {   // children have larger indices than their parent (BvhBuilder pushes them after it)
            for (uint32_t side = 0; side < 2; side++) {
                const uint32_t e = side == 0 ? nodes[i].e0 : nodes[i].e1;
                RefitEntry& d = entries[2 * size_t(i) + side];
                for (int a = 0; a < 3; a++) { d.lo[a] = inf; d.hi[a] = -inf; }
                d.a = d.b = kRefitNone;
                const float* r6 = &s->tree_raw[(2 * size_t(i) + side) * 6];
                if (e & BVH_LEAF) {
                    const uint32_t count = ((e >> 26) & 31u) + 1u, first = e & BVH_INDEX_MASK;
                    if (!(e & BVH_PRIMS) || size_t(first) + count > n_pleaf) return fail(RPT_ERR_STATE, "movable spheres: a scene-tree leaf is not a primitive list");
                    for (uint32_t j = 0; j < count; j++) {
                        const uint32_t code = pleaf[first + j];
                        const auto it = (code >> 28) == K_SPHERE ? slot_of_sph.find(code & 0x0FFFFFFFu) : slot_of_sph.end();
                        if (it != slot_of_sph.end()) {
                            if (d.a == kRefitNone) d.a = it->second;
                            else if (d.b == kRefitNone) d.b = it->second;
                            else return fail(RPT_ERR_UNSUPPORTED, "movable spheres: a scene-tree leaf holds more than two movable spheres");
                            continue;
                        }
                        const float* b = &s->pleaf_box[(size_t(first) + j) * 6];
                        float moved_box[6];
                        const auto obj = (code >> 28) == K_SPHERE ? object_of_sph.find(code & 0x0FFFFFFFu) : object_of_sph.end();
                        const auto at = obj != object_of_sph.end() ? s->dev.moved_centres.find(obj->second) : s->dev.moved_centres.end();
                        if (at != s->dev.moved_centres.end()) {   // a sphere an earlier list moved and this one leaves there: its box is where it is
                            rptu::sphere_item_box(s->objects[obj->second].shape.d.transform[0], at->second.data(), moved_box, moved_box + 3);
                            b = moved_box;
                        }
                        for (int a = 0; a < 3; a++) { d.lo[a] = std::min(d.lo[a], b[a]); d.hi[a] = std::max(d.hi[a], b[3 + a]); }
                    }
                } else if (e >= s->view.top_root) {
                    const uint32_t c = e - s->view.top_root;
                    if (c <= i || c >= n_tree) return fail(RPT_ERR_STATE, "movable spheres: a scene-tree child does not follow its parent");
                    d.a = kRefitInner;
                    d.b = c;
                    height[i] = std::max(height[i], height[c] + 1u);
                } else {   // the root of a mesh tree: nothing below it moves
                    for (int a = 0; a < 3; a++) { d.lo[a] = r6[a]; d.hi[a] = r6[3 + a]; }
                }
            }
        }
        // the bounds of every entry as the refit forms them (the commit's record, unless an earlier list has moved spheres): children first
        for (uint32_t i = n_tree; i-- > 0;)
            for (uint32_t side = 0; side < 2; side++) {
                const RefitEntry& d = entries[2 * size_t(i) + side];
                float* r8 = &raw[(2 * size_t(i) + side) * 8];
                for (int a = 0; a < 3; a++) { r8[a] = d.lo[a]; r8[4 + a] = d.hi[a]; }
                if (d.a == kRefitInner) {
                    const float* c0 = &raw[size_t(d.b) * 16];
                    for (int a = 0; a < 3; a++) { r8[a] = fminf(c0[a], c0[8 + a]); r8[4 + a] = fmaxf(c0[4 + a], c0[12 + a]); }
                } else {
                    for (uint32_t m : {d.a, d.b})
                        if (m != kRefitNone)
                            for (int a = 0; a < 3; a++) { r8[a] = fminf(r8[a], item_box[8 * size_t(m) + a]); r8[4 + a] = fmaxf(r8[4 + a], item_box[8 * size_t(m) + 4 + a]); }
                }
            }
        for (uint32_t i = 0; i < n_tree; i++) n_heights = std::max(n_heights, height[i] + 1u);
        if (n_heights > kRefitMaxHeights) return fail(RPT_ERR_STATE, "movable spheres: the scene tree is higher than its walk's stack");
        height_first.assign(n_heights + 1, 0);
        for (uint32_t i = 0; i < n_tree; i++) height_first[height[i] + 1]++;
        for (uint32_t h = 0; h < n_heights; h++) height_first[h + 1] += height_first[h];
        order.resize(n_tree);
        std::vector<uint32_t> next(height_first.begin(), height_first.end() - 1);
        for (uint32_t i = 0; i < n_tree; i++) order[next[height[i]]++] = i;
    }

    // upload (a failure leaves the scene without movable spheres)
    s->dev.mov = rpt_scene::Device::Movable{};
    auto& m = s->dev.mov;
    auto put = [](rpti::DevMem& d, const void* src, size_t bytes) -> hipError_t {
        hipError_t e = d.reserve(std::max<size_t>(bytes, 16));
        if (e == hipSuccess && bytes) e = hipMemcpy(d.get(), src, bytes, hipMemcpyHostToDevice);
        return e;
    };
    hipError_t e = put(m.d_table, table.data(), table.size() * sizeof(MovableSphere));
    if (e == hipSuccess) e = put(m.d_item_box, item_box.data(), item_box.size() * 4);
    if (e == hipSuccess) e = put(m.d_groups, groups.data(), groups.size() * 4);
    if (e == hipSuccess) e = put(m.d_entries, entries.data(), entries.size() * sizeof(RefitEntry));
    if (e == hipSuccess) e = put(m.d_raw, raw.data(), raw.size() * 4);
    if (e == hipSuccess) e = put(m.d_order, order.data(), order.size() * 4);
    if (e == hipSuccess) e = m.done.create(hipEventDisableTiming);
    if (e != hipSuccess) {
        s->dev.mov = rpt_scene::Device::Movable{};
        return fail(RPT_ERR_DEVICE, std::string("rpt_scene_set_movable_spheres: ") + hipGetErrorString(e));
    }
    m.set = true;
    m.n = n;
    m.objects.assign(objects, objects + n);
    m.n_groups = uint32_t(groups.size());
    m.n_tree = n_tree;
    m.n_heights = n_heights;
    m.height_first = height_first;
    // diagnostics of the counters build that a moved sphere would make stale
    s->view.scan_bound.lo[0] = 1.f;
    s->view.scan_bound.hi[0] = 0.f;
    s->view.n_scan_groups = 0;
    return RPT_OK;
}

int rpt_scene_move_spheres_device(rpt_scene* s, const void* d_centres, const void* d_offsets, void* d_motion, void* hip_stream) {
    if (!s) return fail(RPT_ERR_INVALID, "null scene");
    if (!s->committed) return fail(RPT_ERR_STATE, "rpt_scene_commit must be called first");
    auto& m = s->dev.mov;
    if (!m.set) return fail(RPT_ERR_STATE, "rpt_scene_set_movable_spheres must be called first");
    if (m.n == 0) return RPT_OK;
    if (!d_centres) return fail(RPT_ERR_INVALID, "null centres");
    if (!launch_scene_update_spheres || !launch_scene_update_cull32 || !launch_scene_update_refit)
        return fail(RPT_ERR_UNSUPPORTED, "rpt_scene_move_spheres_device: built without the kernels");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    RPTI_HIP_TRY(hipSetDevice(s->device));
    // behind every pass of the scene that is queued: the launch sets' renders, the feature pass, the last move
    for (auto& ls : s->dev.sets)
        if (ls.used && ls.stream != st) RPTI_HIP_TRY(hipStreamWaitEvent(st, ls.done.get(), 0));
    if (s->dev.feat_used) RPTI_HIP_TRY(hipStreamWaitEvent(st, s->dev.feat_done.get(), 0));
    if (int rc = rpti::wait_for_move(s, st)) return rc;
    SceneUpdateArgs a;
    fill_args(s, a);
    a.centres = static_cast<const double*>(d_centres);
    a.offsets = static_cast<const double*>(d_offsets);
    a.motion = static_cast<double*>(d_motion);
    hipError_t e = launch_scene_update_spheres(a, st);
    if (e == hipSuccess && a.f64) e = launch_scene_update_cull32(a, st);
    if (e == hipSuccess && a.n_tree) e = launch_scene_update_refit(a, s->opt.refit_per_height != 0, st);
    // (recorded after a failed launch too: what was queued before it is what the next pass has to follow)
    const hipError_t er = hipEventRecord(m.done.get(), st);
    m.used = true;
    m.stream = st;
    m.moves++;
    if (s->photon) s->photon_stale = true;
    RPTI_HIP_TRY(e);
    RPTI_HIP_TRY(er);
    return RPT_OK;
}

int rpt_scene_move_spheres(rpt_scene* s, const double* centres, const double* offsets, double* motion) {
    if (!s) return fail(RPT_ERR_INVALID, "null scene");
    if (!s->committed) return fail(RPT_ERR_STATE, "rpt_scene_commit must be called first");
    auto& m = s->dev.mov;
    if (!m.set) return fail(RPT_ERR_STATE, "rpt_scene_set_movable_spheres must be called first");
    if (!centres && m.n) return fail(RPT_ERR_INVALID, "null centres");
    RPTI_HIP_TRY(hipSetDevice(s->device));
    if (m.used) RPTI_HIP_TRY(hipEventSynchronize(m.done.get()));   // (the staging arrays below may still be read by the last move)
    const size_t bytes = size_t(m.n) * 24, n_obj = s->objects.size();
    std::vector<double> table;
    if (m.n) {
        RPTI_HIP_TRY(m.d_centres.reserve(bytes));
        RPTI_HIP_TRY(hipMemcpy(m.d_centres.get(), centres, bytes, hipMemcpyHostToDevice));
        if (offsets) {
            RPTI_HIP_TRY(m.d_offsets.reserve(bytes));
            RPTI_HIP_TRY(hipMemcpy(m.d_offsets.get(), offsets, bytes, hipMemcpyHostToDevice));
        }
    }
    if (motion) {   // identity for every object; the kernel writes the listed ones
        table.assign(n_obj * 24, 0.0);
        for (size_t o = 0; o < n_obj; o++)
            for (int i : {0, 5, 10, 12, 16, 20}) table[o * 24 + i] = 1.0;
        RPTI_HIP_TRY(m.d_motion.reserve(std::max<size_t>(table.size() * 8, 16)));
        if (n_obj) RPTI_HIP_TRY(hipMemcpy(m.d_motion.get(), table.data(), table.size() * 8, hipMemcpyHostToDevice));
    }
    if (int rc = rpt_scene_move_spheres_device(s, m.d_centres.get(), offsets ? m.d_offsets.get() : nullptr, motion ? m.d_motion.get() : nullptr, nullptr)) return rc;
    RPTI_HIP_TRY(hipStreamSynchronize(nullptr));
    if (motion && n_obj) RPTI_HIP_TRY(hipMemcpy(motion, m.d_motion.get(), table.size() * 8, hipMemcpyDeviceToHost));
    return RPT_OK;
}

int rpt_scene_movable_info(rpt_scene* s, uint64_t out[8]) {
    if (!s || !out) return fail(RPT_ERR_INVALID, "null argument");
    if (!s->committed) return fail(RPT_ERR_STATE, "rpt_scene_commit must be called first");
    const auto& m = s->dev.mov;
    out[0] = m.set ? 1 : 0;
    out[1] = m.n;
    out[2] = m.n_tree;
    out[3] = m.n_heights;
    out[4] = m.n_groups;
    out[5] = m.moves;
    out[6] = m.d_table.capacity() + m.d_item_box.capacity() + m.d_groups.capacity() + m.d_entries.capacity() + m.d_raw.capacity() + m.d_order.capacity();
    out[7] = s->dev.arena64 ? 1 : 0;
    return RPT_OK;
}

int rpt_debug_scene_records(rpt_scene* s, uint32_t which, void* out, uint64_t capacity_bytes, uint64_t* bytes) {
    if (!s || !bytes) return fail(RPT_ERR_INVALID, "null argument");
    if (!s->committed) return fail(RPT_ERR_STATE, "rpt_scene_commit must be called first");
    const SceneView& v = s->view;
    const bool f64 = bool(s->dev.arena64);
    const void* src = nullptr;
    uint64_t n = 0;
    switch (which) {
        case RPT_SCENE_RECORDS_SPH: src = v.sph; n = uint64_t(v.n_sph) * sizeof(XfScan); break;
        case RPT_SCENE_RECORDS_SPH_SHADE: src = v.sph_sh; n = uint64_t(v.n_sph) * sizeof(XfShade); break;
        case RPT_SCENE_RECORDS_PBOX:
            src = v.pbox;
            n = (uint64_t(v.n_sph) + v.n_cub + v.n_aabb + v.n_rect_x + v.n_rect_y + v.n_rect_z + v.n_tri + v.n_mono) * sizeof(AabbScan);
            break;
        case RPT_SCENE_RECORDS_TREE_NODES:
            if (v.scene_bvh) { src = v.nodes + v.top_root; n = uint64_t(v.n_nodes - v.top_root) * sizeof(BvhNode); }
            break;
        case RPT_SCENE_RECORDS_TREE_RAW: src = s->dev.mov.d_raw.get(); n = uint64_t(s->dev.mov.n_tree) * 64; break;
        case RPT_SCENE_RECORDS_TREE_ENTRIES: src = s->dev.mov.d_entries.get(); n = uint64_t(s->dev.mov.n_tree) * 2 * sizeof(RefitEntry); break;
        case RPT_SCENE_RECORDS_TREE_ORDER: src = s->dev.mov.d_order.get(); n = uint64_t(s->dev.mov.n_tree) * 4; break;
        case RPT_SCENE_RECORDS_ITEM_BOXES: src = s->dev.mov.d_item_box.get(); n = uint64_t(s->dev.mov.n) * 32; break;
        case RPT_SCENE_RECORDS_TABLE: src = s->dev.mov.d_table.get(); n = uint64_t(s->dev.mov.n) * sizeof(MovableSphere); break;
        case RPT_SCENE_RECORDS_RECS:
        case RPT_SCENE_RECORDS_SHADE:
        case RPT_SCENE_RECORDS_CULL:
        case RPT_SCENE_RECORDS_CULL32: {
            if (!f64) return fail(RPT_ERR_STATE, "rpt_debug_scene_records: this array needs a scene committed with epsilon_policy = 1");
            const uint64_t no = s->view64.n_objects;
            if (which == RPT_SCENE_RECORDS_RECS) { src = s->view64.recs; n = no * sizeof(rpt64::ObjRec); }
            else if (which == RPT_SCENE_RECORDS_SHADE) { src = s->view64.shade; n = no * sizeof(rpt64::ObjShade); }
            else if (which == RPT_SCENE_RECORDS_CULL) { src = s->view64.cull; n = no * sizeof(rpt64::CullBox); }
            else { src = s->view64.cull32; n = ((no + 31) / 32) * sizeof(rpt64::CullBox); }
            break;
        }
        default: return fail(RPT_ERR_INVALID, "rpt_debug_scene_records: unknown array");
    }
    *bytes = n;
    if (!out || n == 0) return RPT_OK;
    if (capacity_bytes < n) return fail(RPT_ERR_INVALID, "output buffer too small");
    RPTI_HIP_TRY(hipSetDevice(s->device));
    RPTI_HIP_TRY(hipDeviceSynchronize());   // (a move may be queued on any stream)
    RPTI_HIP_TRY(hipMemcpy(out, src, n, hipMemcpyDeviceToHost));
    return RPT_OK;
}

}  // extern "C"

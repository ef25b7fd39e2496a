// Test infrastructure (see hip_stubs.h): "moving spheres" on a CPU.  The real rpt_capi.cpp and rpt_scene_update.cpp over malloc-backed
// HIP stubs; the three launchers of scene_update.h run the lane functions of scene_update_lanes.h serially (the cull32 pass as the
// commit's own loop), so that a moved scene can be compared with a fresh commit byte by byte without a device.
// tests/test_scene_update_host.py builds it plain and under ASan + UBSan and reads what it prints and dumps.
//
//   harness <cases.bin> <dump directory>
//
// cases.bin: records of 7 doubles (radius, centre, previous centre).  Sections, each a block of printed lines:
//   flatten     every case committed as a scene of its own, in both modes: the arena bytes of the sphere's records against
//               rpt_sphere_records_host, the motion record against rpt_temporal_motion_record of the two matrices
//   refusals    every refusal of rpt_scene_set_movable_spheres and rpt_scene_move_spheres*, code and message
//   lifecycle   before commit, twice, a move queued on a stream and the scene destroyed behind it, the photon map marked stale
//   update      scenes moved (1 and 3 chained moves, with and without offsets, lists: all, last, none) against fresh commits
//   refit       the 70-sphere scene's tables and nodes dumped for the numpy checks
//   relist      set, move, set with another list, move on the 70-sphere scene: records, motion rows and leaf boxes against fresh commits
#include "hip_stubs.h"
#include "../../rpt_amd/csrc/rpt_capi.cpp"
#include "../../rpt_amd/csrc/rpt_scene_update.cpp"
#include "../../rpt_amd/csrc/scene_update_lanes.h"

#include <cstdio>

static void touch(const void* p) { (void)*static_cast<const volatile char*>(p); }
namespace rptg {
hipError_t launch_render(const RenderArgs& a, int, hipStream_t) { touch(a.slab); touch(a.tiles); return hipSuccess; }
hipError_t render_occupancy(bool, int, int* b, int) { *b = 4; return hipSuccess; }
size_t stream_scratch_bytes_per_block() { return 0; }
int bvh_mode(const SceneView& sc) { return sc.scene_bvh ? 2 : (sc.n_nodes ? 1 : 0); }
hipError_t launch_resolve(const RenderArgs& a, double, double* out, hipStream_t) { touch(a.slab); touch(a.tiles); touch(out); return hipSuccess; }
hipError_t launch_render_f64(const rpt64::Args& q, int, hipStream_t) { touch(q.slab); touch(q.tiles); return hipSuccess; }
hipError_t launch_resolve_f64(const rpt64::Args& q, double, double* out, hipStream_t) { touch(q.slab); touch(q.tiles); touch(out); return hipSuccess; }
hipError_t render_f64_occupancy(bool, int* blocks_per_cu) { *blocks_per_cu = 4; return hipSuccess; }
hipError_t launch_intersect(const SceneView&, uint64_t, const float*, const float*, float*, int32_t*, float*, bool, hipStream_t) { return hipSuccess; }
hipError_t launch_debug_rng(uint64_t, uint32_t, uint32_t, uint32_t, uint32_t*, hipStream_t) { return hipSuccess; }
hipError_t launch_debug_sample_f(const Material&, uint64_t, const float*, const float*, uint64_t, float*, float*, int32_t*, hipStream_t) { return hipSuccess; }
hipError_t launch_debug_bsdf(const Material&, uint64_t, const float*, const float*, const float*, float*, hipStream_t) { return hipSuccess; }
hipError_t launch_buffer_add(uint32_t, const double*, double*, double*, hipStream_t) { return hipSuccess; }
hipError_t launch_buffer_image(uint32_t, uint32_t, uint32_t, uint32_t, const double*, uint8_t*, hipStream_t) { return hipSuccess; }
hipError_t launch_buffer_variance(uint32_t, uint32_t, const double*, const double*, double*, hipStream_t) { return hipSuccess; }
// the kernels of scene_update.hip, serially
static int g_update_launches = 0;
hipError_t launch_scene_update_spheres(const SceneUpdateArgs& a, hipStream_t) {
    g_update_launches++;
    for (uint32_t k = 0; k < a.n; k++) move_sphere_lane(a, k);
    return hipSuccess;
}
hipError_t launch_scene_update_cull32(const SceneUpdateArgs& a, hipStream_t) {
    g_update_launches++;
    for (uint32_t j = 0; j < a.n_groups; j++) {
        const uint32_t g = a.groups[j];
        rpt64::CullBox u{};
        for (int k = 0; k < 3; k++) { u.lo[k] = HUGE_VALF; u.hi[k] = -HUGE_VALF; }
        for (uint32_t i = 32 * g; i < std::min(a.n_objects, 32 * g + 32); i++) {
            if (a.cull[i].unbounded) u.unbounded = 1u;
            if (a.cull[i].slab_test) u.slab_test = 2u;
            for (int k = 0; k < 3; k++) { u.lo[k] = std::min(u.lo[k], a.cull[i].lo[k]); u.hi[k] = std::max(u.hi[k], a.cull[i].hi[k]); }
        }
        if (u.unbounded) for (int k = 0; k < 3; k++) u.lo[k] = u.hi[k] = 0.f;
        a.cull32[g] = u;
    }
    return hipSuccess;
}
hipError_t launch_scene_update_refit(const SceneUpdateArgs& a, bool, hipStream_t) {
    g_update_launches++;
    for (uint32_t h = 0; h < a.n_heights; h++)
        for (uint32_t i = a.height_first[h]; i < a.height_first[h + 1]; i++) {
            refit_entry(a, a.order[i], 0u);
            refit_entry(a, a.order[i], 1u);
        }
    return hipSuccess;
}
}  // namespace rptg
namespace rpti { void photon_release(void*) {} }

namespace {
rpt_material grey() {
    rpt_material m{};
    m.kind = RPT_MAT_LAMBERTIAN;
    m.albedo[0] = m.albedo[1] = m.albedo[2] = 0.7;
    return m;
}
rpt_shape_desc sphere_at(double r, const double* c) {
    rpt_shape_desc d{};
    d.kind = RPT_SHAPE_SPHERE;
    d.has_transform = 1;
    d.transform[0] = d.transform[5] = d.transform[10] = r;
    d.transform[3] = c[0]; d.transform[7] = c[1]; d.transform[11] = c[2];
    d.transform[15] = 1.0;
    return d;
}
int add(rpt_scene* s, const rpt_shape_desc& d) {
    const rpt_material m = grey();
    return rpt_scene_add_object(s, &d, &m);
}
rpt_shape_desc plane_y(double value) {
    rpt_shape_desc d{};
    d.kind = RPT_SHAPE_PLANE;
    d.plane_normal[1] = 1.0;
    d.plane_value = value;
    return d;
}
std::vector<double> g_floor;   // two triangles of 18 doubles (vertices, normals)
rpt_shape_desc floor_quad() {
    if (g_floor.empty()) {
        const double v[4][3] = {{40, -1, 40}, {40, -1, -40}, {-40, -1, -40}, {-40, -1, 40}};
        const int tri[2][3] = {{0, 1, 2}, {0, 2, 3}};
        for (const auto& t : tri) {
            for (int k = 0; k < 3; k++) g_floor.insert(g_floor.end(), v[t[k]], v[t[k]] + 3);
            for (int k = 0; k < 3; k++) { g_floor.push_back(0); g_floor.push_back(1); g_floor.push_back(0); }
        }
    }
    rpt_shape_desc d{};
    d.kind = RPT_SHAPE_MESH;
    d.tris = g_floor.data();
    d.n_tris = 2;
    return d;
}
uint64_t lcg(uint64_t& s) { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return s >> 11; }
double uni(uint64_t& s, double lo, double hi) { return lo + (hi - lo) * (double(lcg(s)) / 9007199254740992.0); }

std::vector<char> records(rpt_scene* s, uint32_t which) {
    uint64_t n = 0;
    if (rpt_debug_scene_records(s, which, nullptr, 0, &n) != RPT_OK) return {};
    std::vector<char> out(n);
    if (n && rpt_debug_scene_records(s, which, out.data(), n, &n) != RPT_OK) out.clear();
    return out;
}
void dump(const std::string& dir, const char* name, const std::vector<char>& bytes) {
    FILE* f = std::fopen((dir + "/" + name).c_str(), "wb");
    if (!f) { std::printf("cannot write %s\n", name); return; }
    if (!bytes.empty()) std::fwrite(bytes.data(), 1, bytes.size(), f);
    std::fclose(f);
}

// ---- flatten: one case, both modes
int flatten_case(const double* cs, int index, int& printed) {
    const double r = cs[0], *c = cs + 1, *p = cs + 4;
    int bad = 0;
    auto report = [&](const char* what) {
        bad++;
        if (printed++ < 12) std::printf("flatten MISMATCH case %d (r=%.17g c=%.17g %.17g %.17g): %s\n", index, r, c[0], c[1], c[2], what);
    };
    float scan[12], shade[12], item[6], pbox[8];
    double inv[12], nrm[9], motion[24];
    rpt64::CullBox cull;
    const int rc_host = rpt_sphere_records_host(r, c, p, scan, shade, item, pbox, inv, nrm, &cull, motion);
    for (int eps = 0; eps < 2; eps++) {
        rpt_scene* s = rpt_scene_create();
        rpt_scene_set_option(s, "epsilon_policy", eps);
        add(s, plane_y(-1.0));
        add(s, sphere_at(r, c));
        if (rpt_scene_commit(s, 0) != RPT_OK) { report(rpt_last_error()); rpt_scene_destroy(s); continue; }
        shade[3] = bits_f(1u);   // the object id of the committed record
        if (std::memcmp(s->view.sph, scan, 48) != 0) report("XfScan");
        if (std::memcmp(s->view.sph_sh, shade, 48) != 0) report("XfShade");
        if (std::memcmp(s->view.pbox, pbox, 32) != 0) report("pbox");
        if (eps) {
            if (std::memcmp(s->view64.recs[1].inv, inv, 96) != 0) report("ObjRec::inv");
            if (std::memcmp(s->view64.shade[1].nrm, nrm, 72) != 0) report("ObjShade::nrm");
            if (std::memcmp(&s->view64.cull[1], &cull, 32) != 0) report("CullBox");
        }
        rpt_scene_destroy(s);
    }
    const rpt_shape_desc cur = sphere_at(r, c), prev = sphere_at(r, p);
    double want[24];
    const int rc_ref = rpt_temporal_motion_record(cur.transform, prev.transform, want);
    if ((rc_ref == RPT_OK) != (rc_host == RPT_OK)) report("motion record: one of the two refuses");
    else if (rc_ref == RPT_OK && std::memcmp(want, motion, sizeof(want)) != 0) report("motion record");
    return bad;
}

// ---- update: a scene of spheres (+ a plane or a floor), moved, against a fresh commit
struct Build {
    int eps = 0;
    bool floor = false;
    double r = 0.2;
    std::vector<double> centres;   // n x 3
};
rpt_scene* commit(const Build& b) {
    rpt_scene* s = rpt_scene_create();
    rpt_scene_set_option(s, "epsilon_policy", b.eps);
    if (b.floor) add(s, floor_quad());
    else add(s, plane_y(-1.0));
    for (size_t i = 0; i < b.centres.size() / 3; i++) add(s, sphere_at(b.r * (1.0 + 0.01 * double(i % 7)), &b.centres[3 * i]));
    if (rpt_scene_commit(s, 0) != RPT_OK) { std::printf("commit failed: %s\n", rpt_last_error()); rpt_scene_destroy(s); return nullptr; }
    return s;
}
std::vector<double> grid_centres(size_t n, uint64_t seed, double jitter) {   // spheres placed apart, jittered
    std::vector<double> c;
    const size_t side = size_t(std::ceil(std::cbrt(double(n))));
    for (size_t i = 0; i < n; i++) {
        c.push_back(double(i % side) + uni(seed, -jitter, jitter));
        c.push_back(double((i / side) % side) + uni(seed, -jitter, jitter));
        c.push_back(double(i / (side * side)) + uni(seed, -jitter, jitter));
    }
    return c;
}
int compare_scenes(const char* name, rpt_scene* a, rpt_scene* b, bool eps) {
    int bad = 0;
    const uint32_t fp32[] = {RPT_SCENE_RECORDS_SPH, RPT_SCENE_RECORDS_SPH_SHADE, RPT_SCENE_RECORDS_PBOX};
    const uint32_t fp64[] = {RPT_SCENE_RECORDS_RECS, RPT_SCENE_RECORDS_SHADE, RPT_SCENE_RECORDS_CULL, RPT_SCENE_RECORDS_CULL32};
    for (uint32_t w : fp32)
        if (records(a, w) != records(b, w)) { bad++; std::printf("update MISMATCH %s: fp32 array %u\n", name, w); }
    if (eps)
        for (uint32_t w : fp64)
            if (records(a, w) != records(b, w)) { bad++; std::printf("update MISMATCH %s: fp64 array %u\n", name, w); }
    return bad;
}
int update_case(const char* name, int eps, bool floor, size_t n, int list /* 0 all, 1 last, 2 none */, int moves, bool offsets) {
    Build A;
    A.eps = eps; A.floor = floor;
    A.centres = grid_centres(n, 11 + n, 0.2);
    rpt_scene* a = commit(A);
    if (!a) return 1;
    std::vector<uint32_t> objs;
    if (list == 0) for (size_t i = 0; i < n; i++) objs.push_back(uint32_t(1 + i));
    if (list == 1) objs.push_back(uint32_t(n));
    int bad = 0;
    if (rpt_scene_set_movable_spheres(a, objs.data(), uint32_t(objs.size())) != RPT_OK) { std::printf("update %s: set failed: %s\n", name, rpt_last_error()); bad++; }
    Build B = A;
    std::vector<double> prev = A.centres;
    for (int mv = 0; mv < moves && !bad; mv++) {
        const std::vector<double> target = grid_centres(n, 100 + uint64_t(mv) + n, 0.3);
        std::vector<double> cen, off, want_c = B.centres;
        for (uint32_t o : objs)
            for (int k = 0; k < 3; k++) {
                const double t = target[3 * (o - 1) + k], d = offsets ? double(int(o % 5)) - 2.0 : 0.0;
                cen.push_back(offsets ? t - d : t);
                off.push_back(d);
                want_c[3 * (o - 1) + k] = offsets ? (t - d) + d : t;
            }
        std::vector<double> motion((n + 1) * 24, -7.0);
        if (rpt_scene_move_spheres(a, cen.data(), offsets ? off.data() : nullptr, motion.data()) != RPT_OK) { std::printf("update %s: move failed: %s\n", name, rpt_last_error()); bad++; break; }
        prev = B.centres;
        B.centres = want_c;
        // the motion table: rpt_temporal_motion_record per object, identity for the ones that are not listed (and for the floor)
        for (size_t o = 0; o <= n; o++) {
            double want[24] = {0};
            if (o == 0) { want[0] = want[5] = want[10] = want[12] = want[16] = want[20] = 1.0; }
            else {
                const double r = B.r * (1.0 + 0.01 * double((o - 1) % 7));
                const rpt_shape_desc cur = sphere_at(r, &B.centres[3 * (o - 1)]), was = sphere_at(r, &prev[3 * (o - 1)]);
                if (rpt_temporal_motion_record(cur.transform, was.transform, want) != RPT_OK) { bad++; std::printf("update %s: reference motion record refused\n", name); }
            }
            if (std::memcmp(want, &motion[o * 24], sizeof(want)) != 0) { bad++; std::printf("update MISMATCH %s: motion row %zu, move %d\n", name, o, mv); }
        }
        rpt_scene* b = commit(B);
        if (!b) { bad++; break; }
        bad += compare_scenes(name, a, b, eps != 0);
        rpt_scene_destroy(b);
    }
    uint64_t info[8] = {0};
    rpt_scene_movable_info(a, info);
    std::printf("update %s: eps=%d n=%zu listed=%zu moves=%d offsets=%d tree_nodes=%llu heights=%llu groups=%llu mismatches=%d\n", name, eps, n, objs.size(), moves,
                int(offsets), (unsigned long long)info[2], (unsigned long long)info[3], (unsigned long long)info[4], bad);
    rpt_scene_destroy(a);
    return bad;
}

void show(const char* what, int rc) { std::printf("refusal %s: rc=%d %s\n", what, rc, rc ? rpt_last_error() : "-"); }
}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) { std::printf("usage: harness <cases.bin> <dump directory>\n"); return 2; }
    int total_bad = 0;
    {   // ---- flatten
        std::vector<double> cases;
        if (FILE* f = std::fopen(argv[1], "rb")) {
            double rec[7];
            while (std::fread(rec, sizeof(double), 7, f) == 7) cases.insert(cases.end(), rec, rec + 7);
            std::fclose(f);
        }
        int bad = 0, printed = 0;
        for (size_t i = 0; i < cases.size() / 7; i++) bad += flatten_case(&cases[7 * i], int(i), printed);
        std::printf("flatten cases=%zu mismatches=%d\n", cases.size() / 7, bad);
        total_bad += bad;
    }
    {   // ---- refusals, in the order include/rpt_hip.h states
        const double c0[3] = {0.5, 0.25, -1.0};
        uint32_t one[1] = {1};
        show("null scene", rpt_scene_set_movable_spheres(nullptr, one, 1));
        rpt_scene* s = rpt_scene_create();
        show("null list", rpt_scene_set_movable_spheres(s, nullptr, 1));
        show("before commit", rpt_scene_set_movable_spheres(s, one, 1));
        show("move before commit", rpt_scene_move_spheres(s, c0, nullptr, nullptr));
        const int i_plane = add(s, plane_y(-1.0));
        const int i_fine = add(s, sphere_at(0.5, c0));
        rpt_shape_desc d = sphere_at(0.5, c0); d.kind = RPT_SHAPE_CUBE; const int i_cube = add(s, d);
        d = sphere_at(0.5, c0); d.transform[1] = 0.1; const int i_shear = add(s, d);
        d = sphere_at(0.5, c0); d.transform[5] = 0.6; const int i_stretch = add(s, d);
        d = sphere_at(0.5, c0); d.has_transform = 0; const int i_bare = add(s, d);
        d = sphere_at(-0.5, c0); const int i_negative = add(s, d);
        d = sphere_at(1e103, c0); const int i_huge = add(s, d);   // r^3 overflows: the scene takes it, a motion record cannot
        std::vector<rpt_shape_desc> kids = {sphere_at(0.2, c0), sphere_at(0.3, c0)};
        rpt_shape_desc g{}; g.kind = RPT_SHAPE_GROUP; g.children = kids.data(); g.n_children = 2; const int i_group = add(s, g);
        const double lc[3] = {0, 5, 0};
        const rpt_shape_desc lamp = sphere_at(1.5, lc);
        rpt_material lm = grey(); lm.emittance = 10.0;
        const int i_twin = add(s, lamp);   // the twin of the light below
        rpt_scene_add_light_object(s, &lamp, &lm);
        d = sphere_at(0.5, c0); d.transform[15] = 2.0; const int i_bottom = add(s, d);
        d = sphere_at(0.5, c0); d.transform[7] = HUGE_VAL; const int i_far = add(s, d);
        std::printf("refusal scene: objects %d %d %d %d %d %d %d %d %d %d %d %d commit=%d\n", i_plane, i_fine, i_cube, i_shear, i_stretch, i_bare, i_negative, i_huge,
                    i_group, i_twin, i_bottom, i_far, rpt_scene_commit(s, 0));
        show("move with no list", rpt_scene_move_spheres(s, c0, nullptr, nullptr));
        show("move_device with no list", rpt_scene_move_spheres_device(s, c0, nullptr, nullptr, nullptr));
        uint32_t l[2];
        auto one_of = [&](const char* what, int index) {
            if (index < 0) { std::printf("refusal %s: the scene refused the object itself\n", what); return; }
            l[0] = uint32_t(index);
            show(what, rpt_scene_set_movable_spheres(s, l, 1));
        };
        one_of("index out of range", 99);
        l[0] = l[1] = uint32_t(i_fine); show("listed twice", rpt_scene_set_movable_spheres(s, l, 2));
        one_of("group", i_group);
        one_of("plane", i_plane);
        one_of("cube", i_cube);
        one_of("light twin", i_twin);
        one_of("no transform", i_bare);
        one_of("off-diagonal", i_shear);
        one_of("not uniform", i_stretch);
        one_of("negative radius", i_negative);
        one_of("bottom row", i_bottom);
        one_of("centre not finite", i_far);
        one_of("radius without a motion record", i_huge);
        l[0] = uint32_t(i_fine); l[1] = uint32_t(i_cube); show("order: the first bad entry is named", rpt_scene_set_movable_spheres(s, l, 2));
        one_of("fine", i_fine);
        show("null centres", rpt_scene_move_spheres(s, nullptr, nullptr, nullptr));
        show("null device centres", rpt_scene_move_spheres_device(s, nullptr, nullptr, nullptr, nullptr));
        uint64_t nbytes = 0;
        show("records: unknown array", rpt_debug_scene_records(s, 77, nullptr, 0, &nbytes));
        show("records: fp64 array of an fp32 scene", rpt_debug_scene_records(s, RPT_SCENE_RECORDS_CULL, nullptr, 0, &nbytes));
        char small[8];
        show("records: buffer too small", rpt_debug_scene_records(s, RPT_SCENE_RECORDS_SPH, small, sizeof small, &nbytes));
        rpt_scene_destroy(s);
    }
    {   // ---- lifecycle
        Build b;
        b.floor = true;
        b.centres = grid_centres(5, 3, 0.1);
        rpt_scene* s = commit(b);
        float boxes[36]; uint64_t masks[5]; uint32_t ng = 9, en = 9;
        rpt_scan_cull_groups(s, boxes, masks, &ng, &en);
        std::printf("lifecycle before set: scan bound %s\n", boxes[0] <= boxes[3] ? "present" : "absent");
        uint32_t l[2] = {1, 2};
        int rc = rpt_scene_set_movable_spheres(s, l, 2);
        rpt_scan_cull_groups(s, boxes, masks, &ng, &en);
        std::printf("lifecycle set: rc=%d scan bound %s groups=%u\n", rc, boxes[0] <= boxes[3] ? "present" : "absent", ng);
        l[0] = 3;
        rc = rpt_scene_set_movable_spheres(s, l, 1);   // replaces the list
        uint64_t info[8];
        rpt_scene_movable_info(s, info);
        std::printf("lifecycle set again: rc=%d listed=%llu moves=%llu\n", rc, (unsigned long long)info[1], (unsigned long long)info[5]);
        s->photon = &info;   // (photon.hip is not linked: any map will do, photon_release is a stub)
        const double to[3] = {7, 8, 9};
        std::vector<double> d_c(to, to + 3);   // "device" memory of the stubs is host memory
        hipStream_t st = reinterpret_cast<hipStream_t>(uintptr_t(0x100));
        rc = rpt_scene_move_spheres_device(s, d_c.data(), nullptr, nullptr, st);
        rpt_scene_movable_info(s, info);
        std::printf("lifecycle move on a stream: rc=%d moves=%llu photon map stale=%d launches=%d\n", rc, (unsigned long long)info[5], int(s->photon_stale), rptg::g_update_launches);
        const std::vector<char> t = records(s, RPT_SCENE_RECORDS_TABLE);
        const rptg::MovableSphere* m = reinterpret_cast<const rptg::MovableSphere*>(t.data());
        std::printf("lifecycle table: sphere=%u object=%u centre=%g %g %g\n", m->sph, m->object, m->centre[0], m->centre[1], m->centre[2]);
        s->photon = nullptr;
        rpt_scene_destroy(s);   // behind the queued move: nothing leaks, nothing is freed twice
        std::printf("lifecycle destroyed\n");
    }
    // ---- update against fresh commits
    for (int eps = 0; eps < 2; eps++) {
        total_bad += update_case("1 sphere", eps, false, 1, 0, 1, false);
        total_bad += update_case("3 spheres and a plane", eps, false, 3, 0, 3, false);
        total_bad += update_case("25, all", eps, false, 25, 0, 3, true);
        total_bad += update_case("25, last", eps, false, 25, 1, 1, false);
        total_bad += update_case("25, none", eps, false, 25, 2, 1, false);
        total_bad += update_case("33", eps, false, 32, 0, 1, false);    // 33 records with the plane: two cull32 groups
        total_bad += update_case("65", eps, false, 64, 0, 3, true);     // a scene tree in the fp32 arena
        total_bad += update_case("65, last", eps, false, 64, 1, 1, false);
        total_bad += update_case("70 over a floor", eps, true, 70, 0, 3, false);
    }
    {   // ---- refit: the tables of the 70-sphere scene for numpy
        const std::string dir = argv[2];
        Build A;
        A.floor = true;
        A.centres = grid_centres(70, 81, 0.2);
        rpt_scene* a = commit(A);
        std::vector<uint32_t> objs;
        for (uint32_t i = 0; i < 70; i += (i % 3 == 2 ? 2 : 1)) objs.push_back(1 + i);   // most of them, not all
        const int rc = rpt_scene_set_movable_spheres(a, objs.data(), uint32_t(objs.size()));
        dump(dir, "nodes_committed.bin", records(a, RPT_SCENE_RECORDS_TREE_NODES));
        dump(dir, "entries.bin", records(a, RPT_SCENE_RECORDS_TREE_ENTRIES));
        dump(dir, "order.bin", records(a, RPT_SCENE_RECORDS_TREE_ORDER));
        dump(dir, "raw_committed.bin", records(a, RPT_SCENE_RECORDS_TREE_RAW));
        dump(dir, "items_committed.bin", records(a, RPT_SCENE_RECORDS_ITEM_BOXES));
        std::vector<double> cen;
        for (uint32_t o : objs) for (int k = 0; k < 3; k++) cen.push_back(A.centres[3 * (o - 1) + k]);
        const int rc_same = rpt_scene_move_spheres(a, cen.data(), nullptr, nullptr);   // onto their own places
        dump(dir, "nodes_same.bin", records(a, RPT_SCENE_RECORDS_TREE_NODES));
        const std::vector<double> target = grid_centres(70, 82, 0.45);
        cen.clear();
        for (uint32_t o : objs) for (int k = 0; k < 3; k++) cen.push_back(target[3 * (o - 1) + k]);
        const int rc_move = rpt_scene_move_spheres(a, cen.data(), nullptr, nullptr);
        dump(dir, "nodes_moved.bin", records(a, RPT_SCENE_RECORDS_TREE_NODES));
        dump(dir, "raw_moved.bin", records(a, RPT_SCENE_RECORDS_TREE_RAW));
        dump(dir, "items_moved.bin", records(a, RPT_SCENE_RECORDS_ITEM_BOXES));
        uint64_t info[8] = {0};
        rpt_scene_movable_info(a, info);
        std::printf("refit set=%d same=%d move=%d listed=%zu tree_nodes=%llu heights=%llu\n", rc, rc_same, rc_move, objs.size(), (unsigned long long)info[2],
                    (unsigned long long)info[3]);
        rpt_scene_destroy(a);
    }
    for (int eps = 0; eps < 2; eps++) {   // ---- relist: set, move, set with another list, move -- against a fresh commit, with the motion rows
        const size_t n = 70;
        Build A;
        A.eps = eps; A.floor = true;
        A.centres = grid_centres(n, 91, 0.2);
        rpt_scene* a = commit(A);
        int bad = 0;
        std::vector<double> now = A.centres;
        auto move = [&](const std::vector<uint32_t>& objs, uint64_t seed, const char* what) {
            const std::vector<double> target = grid_centres(n, seed, 0.3), before = now;
            std::vector<double> cen, motion((n + 1) * 24, -7.0);
            for (uint32_t o : objs)
                for (int k = 0; k < 3; k++) { cen.push_back(target[3 * (o - 1) + k]); now[3 * (o - 1) + k] = target[3 * (o - 1) + k]; }
            if (rpt_scene_set_movable_spheres(a, objs.data(), uint32_t(objs.size())) != RPT_OK || rpt_scene_move_spheres(a, cen.data(), nullptr, motion.data()) != RPT_OK) {
                std::printf("relist %s failed: %s\n", what, rpt_last_error());
                bad++;
                return;
            }
            for (size_t o = 1; o <= n; o++) {   // a listed sphere's row: from where it WAS (wherever an earlier list left it) to where it is
                const double r = A.r * (1.0 + 0.01 * double((o - 1) % 7));
                const rpt_shape_desc cur = sphere_at(r, &now[3 * (o - 1)]), was = sphere_at(r, &before[3 * (o - 1)]);
                double want[24];
                rpt_temporal_motion_record(cur.transform, was.transform, want);
                if (std::memcmp(want, &motion[o * 24], sizeof(want)) != 0) { bad++; std::printf("relist MISMATCH %s: motion row %zu\n", what, o); }
            }
            Build B = A;
            B.centres = now;
            rpt_scene* b = commit(B);
            bad += compare_scenes(what, a, b, eps != 0);
            // the tree: a refit of the tables as they stand reproduces the nodes, and every sphere lies inside its leaf's box
            const std::vector<char> nodes = records(a, RPT_SCENE_RECORDS_TREE_NODES);
            const rptg::BvhNode* nd = reinterpret_cast<const rptg::BvhNode*>(nodes.data());
            for (size_t i = 0; i < nodes.size() / sizeof(rptg::BvhNode); i++)
                for (int side = 0; side < 2; side++) {
                    const uint32_t e = side ? nd[i].e1 : nd[i].e0;
                    if (!(e & rptg::BVH_LEAF)) continue;
                    const float* lo = side ? nd[i].lo1 : nd[i].lo0;
                    const float* hi = side ? nd[i].hi1 : nd[i].hi0;
                    const uint32_t count = ((e >> 26) & 31u) + 1u, first = e & rptg::BVH_INDEX_MASK;
                    for (uint32_t j = 0; j < count; j++) {
                        const uint32_t code = a->view.pleaf[first + j];
                        if ((code >> 28) != rptg::K_SPHERE) continue;
                        const rptg::AabbScan& pb = a->view.pbox[code & 0x0FFFFFFFu];   // padded beyond the sphere's own box by at most 1e-5 of it + 1e-7
                        const float plo[3] = {pb.lo.x, pb.lo.y, pb.lo.z}, phi[3] = {pb.hi.x, pb.hi.y, pb.hi.z};
                        for (int k = 0; k < 3; k++)
                            if (lo[k] > plo[k] + 1e-3f || hi[k] < phi[k] - 1e-3f) { bad++; std::printf("relist MISMATCH %s: sphere record %u lies outside its leaf's box\n", what, code & 0x0FFFFFFFu); }
                    }
                }
            rpt_scene_destroy(b);
        };
        std::vector<uint32_t> all, odd, few = {3, 4, 70};
        for (uint32_t o = 1; o <= n; o++) { all.push_back(o); if (o & 1) odd.push_back(o); }
        move(all, 92, "first list");
        move(odd, 93, "second list: the even spheres stay where the first list moved them");
        move(few, 94, "third list");
        move(all, 95, "fourth list: every sphere again");
        uint64_t info[8] = {0};
        rpt_scene_movable_info(a, info);
        std::printf("relist eps=%d lists=4 tree_nodes=%llu mismatches=%d\n", eps, (unsigned long long)info[2], bad);
        total_bad += bad;
        rpt_scene_destroy(a);
    }
    std::printf("total mismatches=%d\n", total_bad);
    return total_bad ? 1 : 0;
}

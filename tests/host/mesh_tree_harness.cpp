// Test infrastructure for tests/test_host_mesh_tree.py: commits scenes of the reference-epsilon mode with the real rpt_capi.cpp
// (malloc-backed HIP stubs, as flatten_harness.cpp, whose stubs and helpers this file reuses), reads the candidate trees of their meshes
// (f64_layout.h, MeshNode) back from the arena and checks, per tree: every triangle of the mesh is in exactly one leaf; a child's box lies
// inside its parent's; every fp64 vertex lies inside its leaf's fp32 box by at least the padding, and no box has a zero extent; the depth is
// within the limit.  One line per case; with a file name as argument, the first case's tree and triangles are written there (the numpy
// restatement of the walk reads them).
#define main flatten_harness_main
#include "flatten_harness.cpp"
#undef main

#include <functional>

static rpt::Shape quad_grid(int n, double off = 0.0) {   // n x n quads in the plane y = off: every box has a zero extent before the padding
    std::vector<rpt::Triangle> ts;
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) {
            const rpt::Vec3 a{off + i, off, off + j}, b{off + i + 1, off, off + j}, c{off + i + 1, off, off + j + 1}, d{off + i, off, off + j + 1};
            ts.push_back(rpt::Triangle::from_vertices(a, c, b));
            ts.push_back(rpt::Triangle::from_vertices(a, d, c));
        }
    return rpt::mesh(ts);
}
static rpt::Shape few(int n) {
    std::vector<rpt::Triangle> ts = {rpt::Triangle::from_vertices({0, 0, 0}, {1, 0, 0}, {0, 1, 0})};
    if (n > 1) ts.push_back(rpt::Triangle::from_vertices({1, 0, 0}, {1, 1, 0.5}, {0, 1, 0}));
    return rpt::mesh(ts);
}
static rpt::Shape chain(int n) {   // triangles whose sizes grow geometrically: the SAH builder's trees of such input are deep
    std::vector<rpt::Triangle> ts;
    double x = 1.0;
    for (int i = 0; i < n; i++, x *= 1.5) ts.push_back(rpt::Triangle::from_vertices({x, 0, 0}, {1.5 * x, 0, 0}, {x, 0.1 * x, 0.01 * x}));
    return rpt::mesh(ts);
}
static rpt::Shape needle() {
    std::vector<rpt::Triangle> ts;
    for (int i = 0; i < 8; i++) ts.push_back(rpt::Triangle::from_vertices({0, double(i), 0}, {1, double(i), 0}, {0, double(i) + 1, 0}));
    ts.push_back(rpt::Triangle::from_vertices({0, 0, 1}, {1, 0, 1}, {0.5, 1e-6, 1}));
    return rpt::mesh(ts);
}

struct Check {
    uint64_t tris = 0, leaves = 0;
    int depth = 0;
    bool once = true, nested = true, padded = true, thick = true;
};
// walks the tree under `root` (a node index); `seen` counts the visits of every triangle record
static void walk(const rpt_scene* s, uint32_t node, int depth, std::vector<uint32_t>& seen, Check& c) {
    const rpt64::MeshNode& n = s->mnodes64[node];
    c.depth = std::max(c.depth, depth);
    for (int a = 0; a < 3; a++)
        if (!(n.hi[a] > n.lo[a])) c.thick = false;
    if (n.count == 0) {
        for (uint32_t k = n.left_or_first; k < n.left_or_first + 2; k++) {
            const rpt64::MeshNode& ch = s->mnodes64[k];
            for (int a = 0; a < 3; a++)
                if (ch.lo[a] < n.lo[a] || ch.hi[a] > n.hi[a]) c.nested = false;
            walk(s, k, depth + 1, seen, c);
        }
        return;
    }
    c.leaves++;
    double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    for (uint32_t k = 0; k < n.count; k++) {
        const rpt64::Tri& t = s->view64.tris[s->mleaf64[n.left_or_first + k]];
        for (const double* v : {t.v1, t.v2, t.v3})
            for (int a = 0; a < 3; a++) { lo[a] = std::min(lo[a], v[a]); hi[a] = std::max(hi[a], v[a]); }
    }
    double size = 0, mag = 0;
    for (int a = 0; a < 3; a++) { size = std::max(size, hi[a] - lo[a]); mag = std::max(mag, std::max(std::fabs(lo[a]), std::fabs(hi[a]))); }
    const double pad = 0.98 * 1e-5 * (size + mag);   // (2 % for the rounding to fp32, which is 6e-8 of the coordinate)
    for (uint32_t k = 0; k < n.count; k++) {
        const uint32_t j = s->mleaf64[n.left_or_first + k];
        seen.at(j)++;
        c.tris++;
        const rpt64::Tri& t = s->view64.tris[j];
        for (const double* v : {t.v1, t.v2, t.v3})
            for (int a = 0; a < 3; a++)
                if (!(double(n.lo[a]) <= v[a] - pad && v[a] + pad <= double(n.hi[a]))) c.padded = false;
    }
}

static const char* g_dump = nullptr;
static int run(const char* name, const std::function<void(rpt_scene*)>& fill, std::initializer_list<std::pair<const char*, int64_t>> opts) {
    rpt_scene* s = rpt_scene_create();
    rpt_scene_set_option(s, "epsilon_policy", 1);
    for (const auto& o : opts)
        if (rpt_scene_set_option(s, o.first, o.second) != 0) { std::printf("%s option %s refused: %s\n", name, o.first, rpt_last_error()); return 1; }
    fill(s);
    const int rc = rpt_scene_commit(s, 0);
    uint64_t info[8] = {0};
    const int irc = rc == 0 ? rpt_f64_mesh_tree_info(s, info) : 0;
    std::printf("%s rc=%d info_rc=%d meshes=%llu triangles=%llu nodes=%llu depth=%llu bytes=%llu render=%llu photon=%llu min=%llu", name, rc, irc,
                (unsigned long long)info[0], (unsigned long long)info[1], (unsigned long long)info[2], (unsigned long long)info[3],
                (unsigned long long)info[4], (unsigned long long)info[5], (unsigned long long)info[6], (unsigned long long)info[7]);
    if (rc == 0 && info[0] != 0) {
        // every record with a tree: its mesh's triangles, each in exactly one leaf
        Check c;
        std::vector<uint32_t> roots;
        for (uint32_t i = 0; i < s->view64.n_objects; i++) {
            const uint32_t root = s->mroot64[i];
            if (root == 0u || std::find(roots.begin(), roots.end(), root) != roots.end()) continue;
            roots.push_back(root);
            const rpt64::ObjRec& r = s->view64.recs[i];
            std::vector<uint32_t> seen(s->view64.n_obj_tris, 0u);
            walk(s, root - 1u, 0, seen, c);
            for (uint32_t j = 0; j < s->view64.n_obj_tris; j++)
                if (seen[j] != ((j >= r.tri_first && j < r.tri_first + r.tri_count) ? 1u : 0u)) c.once = false;
        }
        std::printf(" trees=%zu walked_triangles=%llu leaves=%llu walked_depth=%d once=%d nested=%d padded=%d thick=%d", roots.size(),
                    (unsigned long long)c.tris, (unsigned long long)c.leaves, c.depth, int(c.once), int(c.nested), int(c.padded), int(c.thick));
        if (g_dump) {   // the first tree: u32 n_nodes, n_leaf, n_tris, root; nodes (8 x 4 bytes); leaf entries (u32); triangles (18 doubles)
            std::FILE* f = std::fopen(g_dump, "wb");
            if (!f) { std::printf(" dump failed\n"); return 1; }
            const uint32_t n_leaf = uint32_t(info[1]);
            const uint32_t head[4] = {uint32_t(info[2]), n_leaf, s->view64.n_obj_tris, roots[0] - 1u};
            std::fwrite(head, 4, 4, f);
            std::fwrite(s->mnodes64, sizeof(rpt64::MeshNode), head[0], f);
            std::fwrite(s->mleaf64, 4, n_leaf, f);
            std::fwrite(s->view64.tris, sizeof(rpt64::Tri), head[2], f);
            std::fclose(f);
            g_dump = nullptr;
        }
    }
    std::printf("\n");
    rpt_scene_destroy(s);
    return 0;
}

int main(int argc, char** argv) {
    using namespace rpt;
    if (argc > 1) g_dump = argv[1];
    int bad = 0;
    const Shape t = torus(24, 12, 0.3, 0.12);   // 576 triangles
    bad |= run("torus", [&](rpt_scene* s) { add(s, t); }, {{"f64_mesh_tree_min", 1}});
    bad |= run("torus_xf", [&](rpt_scene* s) { add(s, t.scale({3.4, 1.7, 2.0}).rotate_y(0.7).translate({100, -3, 2})); }, {{"f64_mesh_tree_min", 1}});
    bad |= run("one", [&](rpt_scene* s) { add(s, few(1)); }, {{"f64_mesh_tree_min", 1}});
    bad |= run("two", [&](rpt_scene* s) { add(s, few(2)); }, {{"f64_mesh_tree_min", 1}});
    bad |= run("grid", [&](rpt_scene* s) { add(s, quad_grid(9)); }, {{"f64_mesh_tree_min", 1}});
    bad |= run("far_grid", [&](rpt_scene* s) { add(s, quad_grid(9, 3e4)); }, {{"f64_mesh_tree_min", 1}});   // (the padding is 0.3 there: fp32 has 2e-3)
    // a mesh that two shapes and a group's child share has one tree; the 12-triangle one beside it has its own at threshold 1
    bad |= run("shared", [&](rpt_scene* s) {
        add(s, t.translate({1, 0, 0}));
        add(s, kdtree({t.scale({0.5, 0.5, 0.5}), sphere().translate({0, 3, 0})}).rotate_z(0.2));
        add(s, torus(3, 2, 0.3, 0.12));
    }, {{"f64_mesh_tree_min", 1}});
    // defaults: the 12-triangle mesh keeps the scan, the torus has a tree; threshold 0 and f64_cull = 0: no tree at all
    bad |= run("default", [&](rpt_scene* s) { add(s, t); add(s, torus(3, 2, 0.3, 0.12)); }, {});
    bad |= run("never", [&](rpt_scene* s) { add(s, t); }, {{"f64_mesh_tree_min", 0}});
    bad |= run("full_scan", [&](rpt_scene* s) { add(s, t); }, {{"f64_mesh_tree_min", 1}, {"f64_cull", 0}});
    // depth: a SAH tree deeper than bvh_max_depth is rebuilt balanced; a mesh whose balanced tree is still too deep is refused
    bad |= run("chain", [&](rpt_scene* s) { add(s, chain(60)); }, {{"f64_mesh_tree_min", 1}, {"bvh_max_depth", 5}, {"bvh_leaf_max", 2}});
    bad |= run("too_deep", [&](rpt_scene* s) { add(s, t); }, {{"f64_mesh_tree_min", 1}, {"bvh_max_depth", 3}});
    // a needle among ordinary triangles: the mesh keeps the scan
    bad |= run("needle", [&](rpt_scene* s) { add(s, needle()); }, {{"f64_mesh_tree_min", 1}});
    // the flavours without the walk keep the scan and say so: a group light, a monomial surface
    bad |= run("group_light", [&](rpt_scene* s) { add(s, t); add(s, kdtree({sphere().translate({0, 3, 0}), cube().translate({2, 3, 0})}), true); }, {{"f64_mesh_tree_min", 1}});
    {   // an fp32 scene has no such trees
        rpt_scene* s = rpt_scene_create();
        add(s, t);
        uint64_t info[8];
        const int before = rpt_f64_mesh_tree_info(s, info);
        const int rc = rpt_scene_commit(s, 0);
        std::printf("fp32 rc=%d before_commit=%d info_rc=%d null=%d\n", rc, before, rpt_f64_mesh_tree_info(s, info), rpt_f64_mesh_tree_info(s, nullptr));
        rpt_scene_destroy(s);
    }
    return bad;
}

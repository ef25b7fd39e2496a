// Test infrastructure for tests/test_host_scan_cull.py: commits a few scenes with the real rpt_capi.cpp (malloc-backed HIP stubs, as
// flatten_harness.cpp, whose stubs and helpers this file reuses) and prints the box a culled primary scan tests before its tail
// (SceneView::scan_tail) and what the counters build classifies trips by -- scan_bound, scan_groups, scan_always -- next to the box
// of every scanned record in the scan's numbering and the shell's.
#define main flatten_harness_main
#include "flatten_harness.cpp"
#undef main

static rpt::Shape quad(double x0, double x1, double y, double z0, double z1) {
    return rpt::polygon({{x1, y, z0}, {x1, y, z1}, {x0, y, z1}, {x0, y, z0}});
}
static void walls(rpt_scene* s) {   // rpt_amd/scenes.py: _cornell_walls
    using rpt::polygon;
    add(s, polygon({{0, 0, 0}, {0, 0, 559.2}, {556, 0, 559.2}, {556, 0, 0}}));
    add(s, polygon({{0, 548.9, 0}, {556, 548.9, 0}, {556, 548.9, 559.2}, {0, 548.9, 559.2}}));
    add(s, polygon({{0, 0, 559.2}, {0, 548.9, 559.2}, {556, 548.9, 559.2}, {556, 0, 559.2}}));
    add(s, polygon({{556, 0, 0}, {556, 0, 559.2}, {556, 548.9, 559.2}, {556, 548.9, 0}}));
    add(s, polygon({{0, 0, 0}, {0, 548.9, 0}, {0, 548.9, 559.2}, {0, 0, 559.2}}));
}
static const double kTwoPi = 6.283185307179586;

static void build(const std::string& name, rpt_scene* s) {
    using namespace rpt;
    if (name == "C3") {   // rpt_amd/scenes.py: lampshade
        walls(s);
        add(s, cube().scale({165, 330, 165}).rotate_y(kTwoPi * (-253.0 / 360.0)).translate({368, 165, 351}));
        add(s, cube().scale({165, 165, 165}).rotate_y(kTwoPi * (-197.0 / 360.0)).translate({185, 82.5, 169}));
        const double cx = 213.0 + 65.0, cy = 548.0, cz = 227.0 + 55.0;
        add(s, cube().scale({10, 140, 125}).translate({cx + 65, cy, cz}));
        add(s, cube().scale({10, 140, 125}).translate({cx - 65, cy, cz}));
        add(s, cube().scale({150, 140, 10}).translate({cx, cy, cz + 52.5}));
        add(s, cube().scale({150, 140, 10}).translate({cx, cy, cz - 52.5}));
        add(s, quad(226, 330, 548.8, 240, 319));
        add(s, quad(226, 330, 548.8, 240, 319), true);
        rpt_scene_add_medium(s, RPT_MEDIUM_HOMOGENEOUS_ISOTROPIC, 0.00005, 0.003);
    } else if (name == "C2") {   // rpt_amd/scenes.py: cornell
        walls(s);
        add(s, cube().scale({165, 330, 165}).rotate_y(kTwoPi * (-253.0 / 360.0)).translate({368, 165, 351}));
        add(s, sphere().scale({80, 80, 80}).rotate_y(kTwoPi * (-197.0 / 360.0)).translate({150, 82.5, 450}));
        add(s, quad(213, 343, 548.8, 227, 332));
        add(s, quad(213, 343, 548.8, 227, 332), true);
    } else if (name == "plane") {   // C2 and a plane: planes are unbounded
        build("C2", s);
        add(s, plane({0, 1, 0}, -10.0));
    } else if (name == "many") {   // 65 scanned records: 64 boxes and the light's rectangle (the scene tree is kept away: scene_bvh_min is raised)
        for (int i = 0; i < 64; i++) add(s, cube().scale({1, 1, 1}).translate({3.0 * (i % 9), 3.0 * (i / 9), 0}));
        add(s, quad(-1, 1, 40, -1, 1));
        add(s, quad(-1, 1, 40, -1, 1), true);
    } else if (name == "notail") {   // spheres and a transformed cube only: nothing behind the shell, nothing to leave out
        add(s, sphere().scale({3, 3, 3}).translate({-7, 0, 0}));
        add(s, cube().scale({2, 3, 1}).rotate_y(0.4).translate({1, 2, 3}));
        add(s, sphere().scale({1, 1, 1}).translate({0, 9, 0}), true);
    } else if (name == "big") {   // one box that is most of the bound among small ones, a sphere and a lone triangle
        add(s, cube().scale({100, 100, 100}).translate({0, 0, 0}));
        for (int i = 0; i < 6; i++) add(s, cube().scale({2, 2, 2}).translate({60.0 + 5.0 * i, 10.0 * i, 0}));
        add(s, sphere().scale({3, 3, 3}).translate({-70, 0, 0}));
        add(s, rpt::mesh({rpt::Triangle::from_vertices({0, 70, 0}, {5, 70, 0}, {0, 70, 5})}));
        add(s, quad(-1, 1, 90, -1, 1));
        add(s, quad(-1, 1, 90, -1, 1), true);
    }
}

static void print_box(const char* key, const float lo[3], const float hi[3]) {
    std::printf(" %s=%.9g,%.9g,%.9g,%.9g,%.9g,%.9g", key, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]);
}

int main() {
    for (const char* name : {"C3", "C2", "plane", "many", "big", "notail"})
        for (int on = 1; on >= 0; on--) {
            rpt_scene* s = rpt_scene_create();
            rpt_scene_set_option(s, "scan_cull", on);
            if (std::string(name) == "many") rpt_scene_set_option(s, "scene_bvh_min", 1000);
            build(name, s);
            const int rc = rpt_scene_commit(s, 0);
            if (rc != 0) { std::printf("%s on=%d rc=%d %s\n", name, on, rc, rpt_last_error()); return 1; }
            const rptg::SceneView& v = s->view;
            const uint32_t n_rect = v.n_rect_x + v.n_rect_y + v.n_rect_z;
            const uint32_t n = v.n_sph + v.n_cub + v.n_aabb + n_rect + v.n_tri;
            std::printf("%s on=%d enabled=%u n=%u n_sph=%u n_cub=%u n_aabb=%u n_rect=%u n_tri=%u n_pln=%u scene_bvh=%u has_shell=%u n_groups=%u always=%llx",
                        name, on, v.scan_cull, n, v.n_sph, v.n_cub, v.n_aabb, n_rect, v.n_tri, v.n_pln, v.scene_bvh, v.has_shell,
                        v.n_scan_groups, (unsigned long long)v.scan_always);
            print_box("bound", v.scan_bound.lo, v.scan_bound.hi);
            print_box("tail", v.scan_tail.lo, v.scan_tail.hi);
            for (uint32_t g = 0; g < v.n_scan_groups; g++) {
                std::printf(" gmask%u=%llx", g, (unsigned long long)v.scan_groups[g].mask);
                char key[16];
                std::snprintf(key, sizeof(key), "gbox%u", g);
                print_box(key, v.scan_groups[g].box.lo, v.scan_groups[g].box.hi);
            }
            if (v.has_shell) { const float lo[3] = {v.shell->lo.x, v.shell->lo.y, v.shell->lo.z}, hi[3] = {v.shell->hi.x, v.shell->hi.y, v.shell->hi.z}; print_box("shell", lo, hi); }
            // the records' own boxes, in the scan's numbering: exact for boxes and rectangles (from the records themselves); for spheres,
            // cubes and triangles the ball-query boxes (pbox), which carry a margin of 1e-5 of their own: the cull's must exceed it
            for (uint32_t i = 0; i < n && i < 64u; i++) {
                char key[16];
                std::snprintf(key, sizeof(key), "rec%u", i);
                float lo[3] = {v.pbox[i].lo.x, v.pbox[i].lo.y, v.pbox[i].lo.z}, hi[3] = {v.pbox[i].hi.x, v.pbox[i].hi.y, v.pbox[i].hi.z};
                const uint32_t first_aabb = v.n_sph + v.n_cub, first_rect = first_aabb + v.n_aabb;
                if (i >= first_aabb && i < first_rect) {
                    const rptg::AabbScan& b = v.aabb[i - first_aabb];
                    lo[0] = b.lo.x; lo[1] = b.lo.y; lo[2] = b.lo.z; hi[0] = b.hi.x; hi[1] = b.hi.y; hi[2] = b.hi.z;
                } else if (i >= first_rect && i < first_rect + n_rect) {
                    const uint32_t k = i - first_rect, axis = k < v.n_rect_x ? 0u : k < v.n_rect_x + v.n_rect_y ? 1u : 2u;
                    const rptg::RectScan& r = v.rect[k];
                    lo[axis] = hi[axis] = r.a.x;
                    lo[(axis + 1) % 3] = r.a.y; hi[(axis + 1) % 3] = r.a.z;
                    lo[(axis + 2) % 3] = r.a.w; hi[(axis + 2) % 3] = r.b.x;
                }
                print_box(key, lo, hi);
            }
            std::printf("\n");
            rpt_scene_destroy(s);
        }
    return 0;
}

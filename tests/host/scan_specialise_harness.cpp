// Test infrastructure for tests/test_host_scan_specialise.py: commits a few scenes with the real rpt_capi.cpp (malloc-backed HIP
// stubs, as flatten_harness.cpp, whose stubs and helpers this file reuses) with the option "scan_specialise" on and off and prints
// what the unmasked scans are told to leave out -- SceneView::sph_yrot / cub_yrot and AabbScan::hi.w -- next to a checksum of
// every scanned array (hi.w cleared) and the lights' twin code ranges, which must not depend on the option.
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
        add(s, cube().scale({10, 140, 125}).translate({cx + 65, cy, cz}));     // right, left: the same y and z extents
        add(s, cube().scale({10, 140, 125}).translate({cx - 65, cy, cz}));
        add(s, cube().scale({150, 140, 10}).translate({cx, cy, cz + 52.5}));   // front, back: the same x and y extents
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
    } else if (name == "mixed") {   // cubes 0..3: about y, about x, sheared, about y with 1e-30 where a zero belongs; sphere 0: about y
        add(s, cube().scale({2, 3, 1}).rotate_y(0.4).translate({1, 2, 3}));
        add(s, cube().scale({2, 3, 1}).rotate_x(0.4).translate({-4, 2, 3}));
        Mat4 shear;
        shear.m[1] = 0.3;   // x += 0.3 y
        add(s, cube().scale({2, 1, 1}).transform(shear).translate({4, -2, 0}));
        Mat4 almost = Mat4::rotation(0.7, {0, 1, 0});
        almost.m[1] = 1e-30;
        add(s, cube().transform(almost).translate({0, 5, 0}));
        add(s, sphere().scale({1, 2, 1}).rotate_y(1.1).translate({0, -3, 1}));
        add(s, quad(-1, 1, 9, -1, 1));
        add(s, quad(-1, 1, 9, -1, 1), true);
    } else if (name == "lastbit") {   // two boxes with the same z extent whose upper y planes differ in the last bit; then a lone fifth box
        add(s, cube().scale({10, 140, 125}).translate({343, 548, 282}));                                  // y: [478, 618]
        add(s, cube().scale({10, 140 + 0x1p-14, 125}).translate({213, 548 + 0x1p-15, 282}));              // y: [478, 618 + 2^-14]
        add(s, cube().scale({10, 140, 125}).translate({343, 548, 282}));                                  // an identical pair: x, y and z
        add(s, cube().scale({10, 140, 125}).translate({343, 548, 282}));
        add(s, cube().scale({10, 140, 125}).translate({343, 548, 282}));
        add(s, quad(-1, 1, 900, -1, 1));
        add(s, quad(-1, 1, 900, -1, 1), true);
    }
}

int main() {
    for (const char* name : {"C3", "C2", "mixed", "lastbit"})
        for (int on = 1; on >= 0; on--) {
            rpt_scene* s = rpt_scene_create();
            rpt_scene_set_option(s, "scan_specialise", on);
            build(name, s);
            const int rc = rpt_scene_commit(s, 0);
            if (rc != 0) { std::printf("%s on=%d rc=%d %s\n", name, on, rc, rpt_last_error()); return 1; }
            const rptg::SceneView& v = s->view;
            std::printf("%s on=%d sph_yrot=%llx cub_yrot=%llx n_sph=%u n_cub=%u n_aabb=%u shared=", name, on, (unsigned long long)v.sph_yrot,
                        (unsigned long long)v.cub_yrot, v.n_sph, v.n_cub, v.n_aabb);
            std::vector<rptg::AabbScan> boxes(v.aabb, v.aabb + v.n_aabb);
            for (rptg::AabbScan& b : boxes) { std::printf("%u,", bits_u(b.hi.w)); b.hi.w = 0.f; }
            const uint32_t n_rect = v.n_rect_x + v.n_rect_y + v.n_rect_z;
            uint64_t h = fnv(v.sph, v.n_sph * sizeof(rptg::XfScan));
            h = fnv(v.cub, v.n_cub * sizeof(rptg::XfScan), h);
            h = fnv(boxes.data(), boxes.size() * sizeof(rptg::AabbScan), h);
            h = fnv(v.rect, n_rect * sizeof(rptg::RectScan), h);
            h = fnv(v.shell, sizeof(rptg::ShellScan), h);
            h = fnv(v.tri, v.n_tri * sizeof(rptg::TriScan), h);
            h = fnv(v.sph_sh, v.n_sph * sizeof(rptg::XfShade), h);
            h = fnv(v.cub_sh, v.n_cub * sizeof(rptg::XfShade), h);
            h = fnv(v.pbox, (v.n_sph + v.n_cub + v.n_aabb + n_rect + v.n_tri) * sizeof(rptg::AabbScan), h);
            std::printf(" records=%016llx twins=", (unsigned long long)h);
            for (uint32_t i = 0; i < v.n_lights; i++) std::printf("%d:%x-%x,", v.lights[i].twin_object, v.lights[i].twin_lo, v.lights[i].twin_hi);
            std::printf(" boxes=");
            for (const rptg::AabbScan& b : boxes)
                std::printf("%08x.%08x.%08x:%08x.%08x.%08x,", bits_u(b.lo.x), bits_u(b.lo.y), bits_u(b.lo.z), bits_u(b.hi.x), bits_u(b.hi.y), bits_u(b.hi.z));
            std::printf("\n");
            rpt_scene_destroy(s);
        }
    return 0;
}

// Test infrastructure for tests/test_scan_shape_host.py: commits C3, C2 and variations of C3 through the real rpt_capi.cpp (malloc-backed
// HIP stubs, as flatten_harness.cpp, whose stubs and helpers this file reuses) and prints, per scene, the scan shape the JIT would
// compile for next to the counts read from the committed view; then cache keys of changed program texts, and -- where libhiprtc can be
// opened -- the lowered name and the resources of the code objects compiled for C3's and C2's shapes.  argv[1]: rpt_amd/csrc.
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

// C3 (rpt_amd/scenes.py: lampshade) with one change; "C2": rpt_amd/scenes.py: cornell.
static void build(const std::string& name, rpt_scene* s) {
    using namespace rpt;
    if (name == "C2") {
        walls(s);
        add(s, cube().scale({165, 330, 165}).rotate_y(kTwoPi * (-253.0 / 360.0)).translate({368, 165, 351}));
        add(s, sphere().scale({80, 80, 80}).rotate_y(kTwoPi * (-197.0 / 360.0)).translate({150, 82.5, 450}));
        add(s, quad(213, 343, 548.8, 227, 332));
        add(s, quad(213, 343, 548.8, 227, 332), true);
        return;
    }
    walls(s);
    if (name == "C3_moved") add(s, cube().scale({120, 300, 90}).rotate_y(0.3).translate({300, 150, 300}));   // another size, angle and place
    else if (name == "C3_general_rotation") add(s, cube().scale({165, 330, 165}).rotate_x(0.2).translate({368, 200, 351}));
    else add(s, cube().scale({165, 330, 165}).rotate_y(kTwoPi * (-253.0 / 360.0)).translate({368, 165, 351}));
    add(s, cube().scale({165, 165, 165}).rotate_y(kTwoPi * (-197.0 / 360.0)).translate({185, 82.5, 169}));
    const double cx = 213.0 + 65.0, cy = 548.0, cz = 227.0 + 55.0;
    add(s, cube().scale({10, 140, 125}).translate({cx + 65, cy, cz}));
    add(s, cube().scale({10, 140, 125}).translate({cx - 65, cy, cz}));
    add(s, cube().scale({150, 140, 10}).translate({cx, cy, cz + 52.5}));
    add(s, cube().scale({150, 140, 10}).translate({cx, cy, cz - 52.5}));
    if (name == "C3_plus_sphere") add(s, sphere().scale({30, 30, 30}).translate({100, 300, 100}));
    if (name == "C3_plus_cube") add(s, cube().scale({30, 30, 30}).rotate_y(0.5).translate({100, 300, 100}));
    if (name == "C3_plus_plane") add(s, plane({0, 1, 0}, -5.0));
    if (name == "C3_plus_box") add(s, cube().scale({30, 30, 30}).translate({100, 300, 100}));
    if (name == "C3_plus_rect_x") add(s, polygon({{100, 100, 100}, {100, 200, 100}, {100, 200, 200}, {100, 100, 200}}));
    if (name == "C3_plus_rect_y") add(s, quad(100, 200, 300, 100, 200));
    if (name == "C3_plus_rect_z") add(s, polygon({{100, 100, 100}, {200, 100, 100}, {200, 200, 100}, {100, 200, 100}}));
    if (name == "C3_plus_triangle") add(s, polygon({{100, 100, 100}, {200, 100, 120}, {150, 200, 140}}));
    add(s, quad(226, 330, 548.8, 240, 319));
    add(s, quad(226, 330, 548.8, 240, 319), true);
    rpt_scene_add_medium(s, RPT_MEDIUM_HOMOGENEOUS_ISOTROPIC, 0.00005, 0.003);
}

int main(int argc, char** argv) {
    const std::string csrc = argc > 1 ? argv[1] : "rpt_amd/csrc";
    rpti::ScanShape c3{}, c2{};
    for (const char* name : {"C3", "C2", "C3_moved", "C3_general_rotation", "C3_no_cull", "C3_plus_sphere", "C3_plus_cube", "C3_plus_plane", "C3_plus_box",
                             "C3_plus_rect_x", "C3_plus_rect_y", "C3_plus_rect_z", "C3_plus_triangle"}) {
        rpt_scene* s = rpt_scene_create();
        if (std::string(name) == "C3_no_cull") rpt_scene_set_option(s, "scan_cull", 0);
        build(name, s);
        const int rc = rpt_scene_commit(s, 0);
        if (rc != 0) { std::printf("%s rc=%d %s\n", name, rc, rpt_last_error()); return 1; }
        const rptg::SceneView& v = s->view;
        rpti::ScanShape h{};
        std::string why;
        const bool in = rpti::scan_shape_of(v, &h, &why);
        std::printf("shape %s in_scope=%d shape=%s view=%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,0x%llxull,0x%llxull;medium=%u\n", name, int(in),
                    rpti::scan_shape_string(h).c_str(), v.n_sph, v.n_cub, v.n_pln, v.n_aabb, v.n_rect_x, v.n_rect_y, v.n_rect_z, v.n_tri, v.has_shell,
                    v.scan_cull, (unsigned long long)v.sph_yrot, (unsigned long long)v.cub_yrot, v.has_medium);
        if (std::string(name) == "C3") c3 = h;
        if (std::string(name) == "C2") c2 = h;
        // the query before any render: the shape, state idle; its argument checks
        int64_t out[8];
        char text[256];
        std::printf("query %s rc=%d", name, rpt_scan_jit_info(s, out, text, sizeof text));
        std::printf(" state=%lld text=%s", (long long)out[0], std::string(text).substr(0, std::string(text).find('\n')).c_str());
        std::printf(" null_scene=%d null_out=%d capacity_without_buffer=%d short=%d", rpt_scan_jit_info(nullptr, out, text, sizeof text),
                    rpt_scan_jit_info(s, nullptr, text, sizeof text), rpt_scan_jit_info(s, out, nullptr, 8), rpt_scan_jit_info(s, out, text, 4));
        std::printf(" short_text=%s\n", text);
        rpt_scene_destroy(s);
    }
    {
        rpt_scene* s = rpt_scene_create();
        int64_t out[8];
        std::printf("options uncommitted=%d set0=%d set2=%d set3=%d setneg=%d\n", rpt_scan_jit_info(s, out, nullptr, 0), rpt_scene_set_option(s, "scan_jit", 0),
                    rpt_scene_set_option(s, "scan_jit", 2), rpt_scene_set_option(s, "scan_jit", 3), rpt_scene_set_option(s, "scan_jit", -1));
        rpt_scene_destroy(s);
    }
    std::vector<std::pair<std::string, std::string>> src;
    std::string why;
    if (!rpti::scan_jit_sources(csrc, &src, &why)) { std::printf("sources failed: %s\n", why.c_str()); return 1; }
    std::printf("sources");
    for (auto& f : src) std::printf(" %s", f.first.c_str());
    std::printf("\n");
    const std::string prog = rpti::scan_jit_program(c3);
    std::string prog1 = prog;
    prog1[prog1.find("RPT_SCAN_SHAPE ") + 15] ^= 1;   // one byte of the program text
    auto src1 = src;
    src1.back().second[src1.back().second.size() / 2] ^= 1;   // one byte of a header
    auto opt1 = rpti::scan_jit_options();
    opt1.back() += " ";
    std::printf("key base=%s again=%s text=%s header=%s options=%s version=%s c2=%s\n", rpti::scan_jit_key(prog, src, rpti::scan_jit_options(), 9, 0).c_str(),
                rpti::scan_jit_key(prog, src, rpti::scan_jit_options(), 9, 0).c_str(), rpti::scan_jit_key(prog1, src, rpti::scan_jit_options(), 9, 0).c_str(),
                rpti::scan_jit_key(prog, src1, rpti::scan_jit_options(), 9, 0).c_str(), rpti::scan_jit_key(prog, src, opt1, 9, 0).c_str(),
                rpti::scan_jit_key(prog, src, rpti::scan_jit_options(), 9, 1).c_str(), rpti::scan_jit_key(rpti::scan_jit_program(c2), src, rpti::scan_jit_options(), 9, 0).c_str());
    // the cache file: written under a temporary name and renamed, read back the same; a truncated one is refused
    if (argc > 2) {
        const std::string dir = argv[2], path = dir + "/sub/x.co";
        std::vector<char> code(1000, 'c'), back;
        std::string low;
        const bool w = rpti::scan_jit_cache_write(dir + "/sub", path, code, "name");
        const bool r = rpti::scan_jit_cache_read(path, &back, &low, &why);
        std::filesystem::resize_file(path, 500);
        const bool t = rpti::scan_jit_cache_read(path, &back, &low, &why);
        std::printf("cache write=%d read=%d same=%d truncated_read=%d why=%s unwritable_write=%d\n", int(w), int(r), int(back.size() == 500 || (low == "name")), int(t),
                    why.c_str(), int(rpti::scan_jit_cache_write("/proc/no/such", "/proc/no/such/x.co", code, "name")));
    }
    for (const rpti::ScanShape* h : {&c3, &c2}) {
        std::vector<char> code;
        std::string low;
        double ms = 0;
        if (!rpti::scan_jit_compile(*h, src, &code, &low, &ms, &why)) { std::printf("compile %s failed: %s\n", h == &c3 ? "C3" : "C2", why.c_str()); continue; }
        int vgprs = -1, scratch = -1;
        const bool res = rpti::scan_jit_resources(code, &vgprs, &scratch);
        std::printf("compile %s ok lowered=%s bytes=%zu resources=%d vgprs=%d scratch=%d ms=%.0f\n", h == &c3 ? "C3" : "C2", low.c_str(), code.size(), int(res), vgprs, scratch, ms);
    }
    return 0;
}

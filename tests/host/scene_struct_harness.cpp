// Test infrastructure for tests/test_scene_struct_host.py: commits C3, C2 and variations of C3 through the real rpt_capi.cpp (malloc-backed
// HIP stubs, as flatten_harness.cpp, whose stubs and helpers this file reuses) and prints, per scene, the structure block the scan JIT
// would compile with -- its text form, the constants behind "#define RPT_SCENE_STRUCT" and the cache key of the program -- and, where
// libhiprtc can be opened, the resources and instruction counts of C3's and C2's code objects with and without the block.
// argv[1]: rpt_amd/csrc.
#define main flatten_harness_main
#include "flatten_harness.cpp"
#undef main

static void addm(rpt_scene* s, const rpt::Shape& sh, int kind, double r, double g, double b, double emit = 0.0, bool light = false) {
    rpt_shape_desc d = sh.desc();
    rpt_material m{};
    m.kind = kind;
    m.albedo[0] = r; m.albedo[1] = g; m.albedo[2] = b;
    m.emittance = emit;
    m.shininess = 20.0;
    m.ior = 1.5;
    if (light) { if (rpt_scene_add_light_object(s, &d, &m) != 0) std::printf("light rejected: %s\n", rpt_last_error()); }
    else if (rpt_scene_add_object(s, &d, &m) < 0) std::printf("object rejected: %s\n", rpt_last_error());
}
static rpt::Shape quad(double x0, double x1, double y, double z0, double z1) {
    return rpt::polygon({{x1, y, z0}, {x1, y, z1}, {x0, y, z1}, {x0, y, z0}});
}
static void walls(rpt_scene* s, double grey) {   // rpt_amd/scenes.py: _cornell_walls
    using rpt::polygon;
    addm(s, polygon({{0, 0, 0}, {0, 0, 559.2}, {556, 0, 559.2}, {556, 0, 0}}), RPT_MAT_LAMBERTIAN, grey, grey, grey);
    addm(s, polygon({{0, 548.9, 0}, {556, 548.9, 0}, {556, 548.9, 559.2}, {0, 548.9, 559.2}}), RPT_MAT_LAMBERTIAN, grey, grey, grey);
    addm(s, polygon({{0, 0, 559.2}, {0, 548.9, 559.2}, {556, 548.9, 559.2}, {556, 0, 559.2}}), RPT_MAT_LAMBERTIAN, grey, grey, grey);
    addm(s, polygon({{556, 0, 0}, {556, 0, 559.2}, {556, 548.9, 559.2}, {556, 548.9, 0}}), RPT_MAT_LAMBERTIAN, 0.7, 0.0, 0.0);
    addm(s, polygon({{0, 0, 0}, {0, 548.9, 0}, {0, 548.9, 559.2}, {0, 0, 559.2}}), RPT_MAT_LAMBERTIAN, 0.0, 0.7, 0.0);
}
static const double kTwoPi = 6.283185307179586;

// C3 (rpt_amd/scenes.py: lampshade) with one change; "C2": rpt_amd/scenes.py: cornell.
static void build(const std::string& name, rpt_scene* s) {
    using namespace rpt;
    const int L = RPT_MAT_LAMBERTIAN;
    if (name == "C2") {
        walls(s, 0.67);
        addm(s, cube().scale({165, 330, 165}).rotate_y(kTwoPi * (-253.0 / 360.0)).translate({368, 165, 351}), L, 0.67, 0.67, 0.67);
        addm(s, sphere().scale({80, 80, 80}).rotate_y(kTwoPi * (-197.0 / 360.0)).translate({150, 82.5, 450}), L, 0.67, 0.67, 0.67);
        addm(s, quad(213, 343, 548.8, 227, 332), L, 1, 1, 1, 100.0);
        addm(s, quad(213, 343, 548.8, 227, 332), L, 1, 1, 1, 100.0, true);
        return;
    }
    const bool moved = name == "C3_values";   // other colours, sizes, places and another light quad: values only
    walls(s, moved ? 0.5 : 0.67);
    if (moved) addm(s, cube().scale({120, 300, 90}).rotate_y(0.3).translate({300, 150, 300}), L, 0.2, 0.3, 0.4);
    else addm(s, cube().scale({165, 330, 165}).rotate_y(kTwoPi * (-253.0 / 360.0)).translate({368, 165, 351}), name == "C3_one_mirror" ? RPT_MAT_MIRROR : L, 0.67, 0.67, 0.67);
    addm(s, cube().scale({165, 165, 165}).rotate_y(kTwoPi * (-197.0 / 360.0)).translate({185, 82.5, 169}), L, 0.67, 0.67, 0.67);
    const double cx = 213.0 + 65.0 + (moved ? 3.0 : 0.0), cy = 548.0, cz = 227.0 + 55.0;
    // the shade: two pairs of boxes; each pair has its x or z slab apart and the two others in common
    addm(s, cube().scale({10, 140, 125}).translate({cx + 65, cy, cz}), L, 0.7, 0.7, 0.0);
    addm(s, cube().scale({10, name == "C3_other_slabs" ? 120.0 : 140.0, 125}).translate({cx - 65, cy, cz}), L, 0.7, 0.7, 0.0);   // (another height: the pair's y slabs differ)
    addm(s, cube().scale({150, 140, 10}).translate({cx, cy, cz + 52.5}), L, 0.7, 0.7, 0.0);
    addm(s, cube().scale({150, 140, 10}).translate({cx, cy, cz - 52.5}), L, 0.7, 0.7, 0.0);
    if (name == "C3_sphere_light") {
        const Shape lamp = sphere().scale({20, 20, 20}).translate({278, 500, 280});
        addm(s, lamp, L, 1, 1, 1, 150.0);
        addm(s, lamp, L, 1, 1, 1, 150.0, true);
    } else {
        const double dx = moved ? 5.0 : 0.0;
        addm(s, quad(226 + dx, 330 + dx, 548.8, 240, 319), L, 1, 1, 1, moved ? 80.0 : 150.0);
        addm(s, quad(226 + dx, 330 + dx, 548.8, 240, 319), L, 1, 1, 1, moved ? 80.0 : 150.0, true);
    }
    if (name == "C3_plus_ambient") { const double c[3] = {0.1, 0.1, 0.1}; rpt_scene_add_light_ambient(s, c); }
    if (name == "C3_six_lights")
        for (int i = 0; i < 5; i++) { const double c[3] = {0.01, 0.01, 0.01}; rpt_scene_add_light_ambient(s, c); }
    if (name != "C3_no_medium") rpt_scene_add_medium(s, name == "C3_glowing_fog_all_groups" ? RPT_MEDIUM_COLORED_GLOWING_FOG : RPT_MEDIUM_HOMOGENEOUS_ISOTROPIC, 0.00005, 0.003);
}

// Static instruction count of a code object's one kernel: words of its .text are not decoded here -- the size of the section is what
// a reader can compare between two builds (bytes), next to VGPRs and scratch.
static size_t text_bytes(const std::vector<char>& code) {
    // ELF64: section headers at e_shoff, names in section e_shstrndx
    if (code.size() < 64 || std::memcmp(code.data(), "\177ELF", 4) != 0) return 0;
    auto rd = [&](size_t off, int n) { uint64_t v = 0; if (off + size_t(n) <= code.size()) std::memcpy(&v, code.data() + off, size_t(n)); return v; };
    const uint64_t shoff = rd(0x28, 8), shentsize = rd(0x3A, 2), shnum = rd(0x3C, 2), shstrndx = rd(0x3E, 2);
    if (!shoff || shentsize < 64 || shstrndx >= shnum) return 0;
    const uint64_t stroff = rd(size_t(shoff + shstrndx * shentsize + 0x18), 8);
    for (uint64_t i = 0; i < shnum; i++) {
        const size_t h = size_t(shoff + i * shentsize);
        const uint64_t name = rd(h, 4), size = rd(h + 0x20, 8);
        const size_t at = size_t(stroff + name);
        if (at + 6 <= code.size() && std::memcmp(code.data() + at, ".text", 6) == 0) return size_t(size);
    }
    return 0;
}

int main(int argc, char** argv) {
    const std::string csrc = argc > 1 ? argv[1] : "rpt_amd/csrc";
    std::vector<std::pair<std::string, std::string>> src;
    std::string why;
    if (!rpti::scan_jit_sources(csrc, &src, &why)) { std::printf("sources failed: %s\n", why.c_str()); return 1; }
    rpti::ScanShape shape_c3{}, shape_c2{};
    rpti::SceneStruct struct_c3{}, struct_c2{};
    for (const char* name : {"C3", "C2", "C3_values", "C3_one_mirror", "C3_sphere_light", "C3_other_slabs", "C3_plus_ambient", "C3_six_lights", "C3_no_medium", "C3_all_groups", "C3_glowing_fog_all_groups"}) {
        rpt_scene* s = rpt_scene_create();
        const bool all = std::string(name).find("_all_groups") != std::string::npos;   // (the groups outside the default as well)
        if (all) setenv("RPT_SCAN_STRUCT_GROUPS", "31", 1);
        build(name, s);
        const int rc = rpt_scene_commit(s, 0);
        if (all) unsetenv("RPT_SCAN_STRUCT_GROUPS");
        if (rc != 0) { std::printf("%s rc=%d %s\n", name, rc, rpt_last_error()); return 1; }
        rpti::ScanShape h{};
        const bool in = rpti::scan_shape_of(s->view, &h, &why);
        const rpti::SceneStruct& t = s->jit.structure;
        char text[512], tiny[8];
        const int qrc = rpt_scan_jit_structure(s, text, sizeof text);
        const int short_rc = rpt_scan_jit_structure(s, tiny, sizeof tiny);
        const std::string prog = rpti::scan_jit_program(h, t);
        std::printf("struct %s in_scope=%d shape=%s structure=%s query_rc=%d query=%s short_rc=%d short=%s null=%d key=%s begins_with_shape_block=%d\n", name, int(in),
                    rpti::scan_shape_string(h).c_str(), rpti::scan_struct_string(t).c_str(), qrc, text, short_rc, tiny, rpt_scan_jit_structure(s, nullptr, 8),
                    rpti::scan_jit_key(prog, src, rpti::scan_jit_options(), 9, 0).c_str(),
                    int(prog.rfind("#define RPT_SCAN_SHAPE " + rpti::scan_shape_constants(h) + "\n#define RPT_SCENE_STRUCT ", 0) == 0));
        if (std::string(name) == "C3") { shape_c3 = h; struct_c3 = t; }
        if (std::string(name) == "C2") { shape_c2 = h; struct_c2 = t; }
        rpt_scene_destroy(s);
    }
    {   // every group alone: the fields of the others are zero, whatever the scene holds
        rpt_scene* s = rpt_scene_create();
        build("C3", s);
        if (rpt_scene_commit(s, 0) != 0) return 1;
        for (uint32_t g : {0u, 1u, 2u, 4u, 8u, 16u}) {
            setenv("RPT_SCAN_STRUCT_GROUPS", std::to_string(g).c_str(), 1);
            rpt_scene* q = rpt_scene_create();
            build("C3", q);
            if (rpt_scene_commit(q, 0) != 0) return 1;
            std::printf("groups %u structure=%s\n", g, rpti::scan_struct_string(q->jit.structure).c_str());
            rpt_scene_destroy(q);
        }
        unsetenv("RPT_SCAN_STRUCT_GROUPS");
        rpt_scene_destroy(s);
    }
    std::printf("program %s", rpti::scan_jit_program(shape_c3, struct_c3).c_str());
    struct Case { const char* name; const rpti::ScanShape* h; const rpti::SceneStruct* t; };
    for (const Case& c : {Case{"C3", &shape_c3, &struct_c3}, Case{"C3_shape_only", &shape_c3, nullptr}, Case{"C2", &shape_c2, &struct_c2}, Case{"C2_shape_only", &shape_c2, nullptr}}) {
        std::vector<char> code;
        std::string low;
        double ms = 0;
        if (!rpti::scan_jit_compile(*c.h, c.t, src, &code, &low, &ms, &why)) { std::printf("compile %s failed: %s\n", c.name, why.c_str()); continue; }
        int vgprs = -1, scratch = -1;
        const bool res = rpti::scan_jit_resources(code, &vgprs, &scratch);
        std::printf("compile %s ok lowered=%s bytes=%zu text_bytes=%zu resources=%d vgprs=%d scratch=%d ms=%.0f\n", c.name, low.c_str(), code.size(), text_bytes(code), int(res),
                    vgprs, scratch, ms);
    }
    return 0;
}

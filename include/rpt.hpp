// rpt.hpp — header-only C++17 mirror of rpt's builder API over the C ABI of rpt_hip.h.
//
// rpt is a Rust crate; no Rust toolchain exists in this environment, so the host layer above the
// C ABI is C++ with the reference's names, argument meaning and builder style (methods take the
// object by value and return it, as `fn width(mut self, ..) -> Self` does).  Reference lines:
//   Scene/SceneAdd scene.rs:12-81   Object object.rs:10-31   Light light.rs:7-19
//   Material material.rs:8-97       Medium medium.rs:78-122  Camera camera.rs:9-62
//   shapes shape.rs:102-314         Renderer renderer.rs:23-156   Buffer/Filter buffer.rs:6-108
//   hex_color/color_bytes color.rs:10-24
// Errors: where the reference panics (assert!/expect/unimplemented!), this layer throws rpt::Error.
#pragma once
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <istream>
#include <iterator>
#include <sstream>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "rpt_hip.h"

namespace rpt {

struct Error : std::runtime_error {
    using std::runtime_error::runtime_error;
};
inline void check(int rc) {
    if (rc < 0) throw Error(std::string("rpt error ") + std::to_string(rc) + ": " + rpt_last_error());
}

using Vec3 = std::array<double, 3>;
using Color = Vec3;
inline Vec3 vec3(double x, double y, double z) { return {x, y, z}; }
inline Vec3 operator+(Vec3 a, Vec3 b) { return {a[0] + b[0], a[1] + b[1], a[2] + b[2]}; }
inline Vec3 operator-(Vec3 a, Vec3 b) { return {a[0] - b[0], a[1] - b[1], a[2] - b[2]}; }
inline Vec3 operator*(double s, Vec3 a) { return {s * a[0], s * a[1], s * a[2]}; }
inline double dot(Vec3 a, Vec3 b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
inline Vec3 cross(Vec3 a, Vec3 b) {
    return {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
}
inline Vec3 normalize(Vec3 a) {
    double l = std::sqrt(dot(a, a));
    return {a[0] / l, a[1] / l, a[2] / l};
}

// ---- color.rs
inline Color hex_color(uint32_t x) {
    auto ch = [](uint32_t c) { return std::pow(double(c) / 255.0, 2.2); };
    return {ch((x >> 16) & 0xff), ch((x >> 8) & 0xff), ch(x & 0xff)};
}
inline std::array<uint8_t, 3> color_bytes(const Color& c) {
    std::array<uint8_t, 3> o{};
    for (int i = 0; i < 3; i++) {
        double t = std::pow(std::fmin(std::fmax(c[i], 0.0), 1.0), 1.0 / 2.2) * 255.0;
        o[i] = (t != t || t <= 0.0) ? 0 : (t >= 255.0 ? 255 : uint8_t(t));  // `as u8`: truncating, saturating
    }
    return o;
}

// ---- 4x4 row-major matrices (glm::translate / scale / rotate of the identity)
struct Mat4 {
    std::array<double, 16> m{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    Mat4 operator*(const Mat4& o) const {
        Mat4 r;
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 4; j++) {
                double s = 0;
                for (int k = 0; k < 4; k++) s += m[i * 4 + k] * o.m[k * 4 + j];
                r.m[i * 4 + j] = s;
            }
        return r;
    }
    static Mat4 translation(Vec3 v) {
        Mat4 r;
        r.m[3] = v[0]; r.m[7] = v[1]; r.m[11] = v[2];
        return r;
    }
    static Mat4 scaling(Vec3 v) {
        Mat4 r;
        r.m[0] = v[0]; r.m[5] = v[1]; r.m[10] = v[2];
        return r;
    }
    static Mat4 rotation(double angle, Vec3 axis) {
        Vec3 a = normalize(axis);
        double c = std::cos(angle), s = std::sin(angle), x = a[0], y = a[1], z = a[2];
        Mat4 r;
        r.m = {c + x * x * (1 - c), x * y * (1 - c) - z * s, x * z * (1 - c) + y * s, 0,
               y * x * (1 - c) + z * s, c + y * y * (1 - c), y * z * (1 - c) - x * s, 0,
               z * x * (1 - c) - y * s, z * y * (1 - c) + x * s, c + z * z * (1 - c), 0,
               0, 0, 0, 1};
        return r;
    }
};

// ---- shapes (shape.rs, shape/*.rs).  One value type covers Sphere / Cube / Plane / Mesh / MonomialSurface and
//      `Transformed<T>`; chained transforms left-multiply and never nest (shape.rs:232-285).
struct Triangle {
    Vec3 v1, v2, v3, n1, n2, n3;
    static Triangle from_vertices(Vec3 a, Vec3 b, Vec3 c) {
        Vec3 n = normalize(cross(b - a, c - a));
        return {a, b, c, n, n, n};
    }
};
class Shape {
  public:
    int kind = RPT_SHAPE_SPHERE;
    bool has_transform = false;
    Mat4 matrix;
    Vec3 plane_normal{0, 0, 0};
    double plane_value = 0;
    std::vector<double> tris;  // 18 doubles per triangle
    std::vector<Shape> children;  // RPT_SHAPE_GROUP: KdTree<Box<dyn Bounded>> (kdtree.rs:103-146)

    Shape translate(Vec3 v) const { return wrap(Mat4::translation(v)); }
    Shape scale(Vec3 v) const { return wrap(Mat4::scaling(v)); }
    Shape rotate(double angle, Vec3 axis) const { return wrap(Mat4::rotation(angle, axis)); }
    Shape rotate_x(double a) const { return wrap(Mat4::rotation(a, {1, 0, 0})); }
    Shape rotate_y(double a) const { return wrap(Mat4::rotation(a, {0, 1, 0})); }
    Shape rotate_z(double a) const { return wrap(Mat4::rotation(a, {0, 0, 1})); }
    Shape transform(const Mat4& t) const { return wrap(t); }

    rpt_shape_desc desc() const {
        rpt_shape_desc d{};
        d.kind = kind;
        d.has_transform = has_transform ? 1 : 0;
        for (int i = 0; i < 16; i++) d.transform[i] = matrix.m[i];
        for (int i = 0; i < 3; i++) d.plane_normal[i] = plane_normal[i];
        d.plane_value = plane_value;
        d.tris = tris.empty() ? nullptr : tris.data();
        d.n_tris = tris.size() / 18;
        child_descs_.clear();
        for (const Shape& c : children) child_descs_.push_back(c.desc());  // valid while *this is alive and unchanged
        d.children = child_descs_.empty() ? nullptr : child_descs_.data();
        d.n_children = child_descs_.size();
        return d;
    }

    // MonomialSurface::closest_point / closest_point_precise (monomial_surface.rs:126-178) of the bare surface: the closest of 201 /
    // 20,001 curve samples, a host function whose arithmetic rpt_hip.h states.
    Vec3 closest_point(Vec3 p, bool precise = false) const {
        if (kind != RPT_SHAPE_MONOMIAL || has_transform) throw Error("closest_point: not a bare monomial surface");
        Vec3 out{};
        check(rpt_monomial_closest_point(plane_normal[0], p.data(), precise ? 1 : 0, out.data()));
        return out;
    }
    Vec3 closest_point_precise(Vec3 p) const { return closest_point(p, true); }

  private:
    mutable std::vector<rpt_shape_desc> child_descs_;
    Shape wrap(const Mat4& t) const {
        Shape s = *this;
        s.matrix = has_transform ? t * matrix : t;
        s.has_transform = true;
        return s;
    }
};
using Mesh = Shape;  // `Mesh = KdTree<Triangle>` (shape/mesh.rs:103); the accelerator is built in the library
inline Shape sphere() { return Shape{}; }
inline Shape cube() {
    Shape s;
    s.kind = RPT_SHAPE_CUBE;
    return s;
}
inline Shape plane(Vec3 normal, double value) {
    Shape s;
    s.kind = RPT_SHAPE_PLANE;
    s.plane_normal = normal;
    s.plane_value = value;
    return s;
}
inline Shape monomial_surface(double height, double exp) {  // shape.rs:292-295; y = height (x^2 + z^2)^2, x^2 + z^2 <= 1
    Shape s;                                                 // (intersection hard-codes the exponent 4, as the reference does)
    s.kind = RPT_SHAPE_MONOMIAL;
    s.plane_normal = {height, exp, 0};
    return s;
}
inline Shape mesh(const std::vector<Triangle>& ts) {  // Mesh::new
    Shape s;
    s.kind = RPT_SHAPE_MESH;
    for (const Triangle& t : ts)
        for (const Vec3* v : {&t.v1, &t.v2, &t.v3, &t.n1, &t.n2, &t.n3})
            for (double c : *v) s.tris.push_back(c);
    return s;
}
inline Shape kdtree(std::vector<Shape> shapes) {  // KdTree::new over bounded shapes (examples/fractal_spheres.rs:45)
    Shape s;
    s.kind = RPT_SHAPE_GROUP;
    for (const Shape& c : shapes)
        if (c.kind == RPT_SHAPE_PLANE) throw std::invalid_argument("Plane is not Bounded and cannot be put in a KdTree");
    if (shapes.empty()) throw std::invalid_argument("KdTree needs at least one shape");
    s.children = std::move(shapes);
    return s;
}
inline Shape polygon(const std::vector<Vec3>& verts) {  // shape.rs:308-314
    std::vector<Triangle> ts;
    for (size_t i = 1; i + 1 < verts.size(); i++) ts.push_back(Triangle::from_vertices(verts[0], verts[i], verts[i + 1]));
    return mesh(ts);
}

// ---- io.rs: host-only mesh loaders (they only produce the triangle array the hot path consumes)
namespace io_detail {
inline bool parse_index(const std::string& v, size_t length, long& out) {  // io.rs:12-20
    if (v.empty()) return false;
    char* end = nullptr;
    long i = std::strtol(v.c_str(), &end, 10);
    if (end == v.c_str() || *end != '\0') return false;
    out = i > 0 ? i - 1 : long(length) + i;
    return true;
}
}  // namespace io_detail
// load_obj (io.rs:28-74, faces :164-201): `v`, `vn`, `f` with a, a/b, a//c, a/b/c indices (1-based, negative =
// relative to the end), polygons fan-triangulated, face normals when a corner lacks a `vn`; other commands skipped.
inline Shape load_obj(std::istream& in) {
    std::vector<Vec3> vertices, normals;
    std::vector<Triangle> tris;
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string cmd;
        if (!(ls >> cmd) || cmd[0] == '#') continue;
        if (cmd == "v" || cmd == "vn") {
            double x, y, z;
            if (!(ls >> x >> y >> z)) throw Error("Invalid point in .OBJ file");
            (cmd == "v" ? vertices : normals).push_back({x, y, z});
        } else if (cmd == "f") {
            std::vector<long> vi, vni;
            std::string tok;
            while (ls >> tok) {
                std::string part[3];
                size_t k = 0, start = 0;
                for (size_t c = 0; c <= tok.size() && k < 3; c++)
                    if (c == tok.size() || tok[c] == '/') { part[k++] = tok.substr(start, c - start); start = c + 1; }
                long v = 0, n = -1;
                if (!io_detail::parse_index(part[0], vertices.size(), v) || v < 0 || size_t(v) >= vertices.size())
                    throw Error("Invalid vertex index");
                if (!io_detail::parse_index(part[2], normals.size(), n)) n = -1;
                vi.push_back(v);
                vni.push_back(n);
            }
            for (size_t i = 1; i + 1 < vi.size(); i++) {
                const size_t c[3] = {0, i, i + 1};
                const Vec3 &v1 = vertices[vi[c[0]]], &v2 = vertices[vi[c[1]]], &v3 = vertices[vi[c[2]]];
                if (vni[c[0]] < 0 || vni[c[1]] < 0 || vni[c[2]] < 0) tris.push_back(Triangle::from_vertices(v1, v2, v3));
                else tris.push_back({v1, v2, v3, normals.at(vni[c[0]]), normals.at(vni[c[1]]), normals.at(vni[c[2]])});
            }
        }
    }
    return mesh(tris);
}
// load_stl (io.rs:264-364): ASCII or binary STL, face normals recomputed from the vertices.
inline Shape load_stl(std::istream& in) {
    std::string data((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    std::vector<Triangle> tris;
    const size_t first = data.find_first_not_of(" \t\r\n");
    const bool ascii = first != std::string::npos && data.compare(first, 5, "solid") == 0 &&
                       data.substr(0, std::min<size_t>(data.size(), 2048)).find("facet") != std::string::npos;
    if (ascii) {
        std::istringstream ss(data);
        std::string word;
        std::vector<Vec3> pts;
        while (ss >> word)
            if (word == "vertex") {
                double x, y, z;
                if (!(ss >> x >> y >> z)) throw Error("Invalid vertex in .STL file");
                pts.push_back({x, y, z});
                if (pts.size() == 3) { tris.push_back(Triangle::from_vertices(pts[0], pts[1], pts[2])); pts.clear(); }
            }
    } else {
        if (data.size() < 84) throw Error("Invalid binary .STL file");
        uint32_t n;
        std::memcpy(&n, data.data() + 80, 4);
        if (data.size() < 84 + size_t(n) * 50) throw Error("Truncated binary .STL file");
        for (uint32_t i = 0; i < n; i++) {
            float f[12];
            std::memcpy(f, data.data() + 84 + size_t(i) * 50, 48);
            tris.push_back(Triangle::from_vertices({f[3], f[4], f[5]}, {f[6], f[7], f[8]}, {f[9], f[10], f[11]}));
        }
    }
    return mesh(tris);
}

// ---- material.rs
struct Material {
    int kind = RPT_MAT_LAMBERTIAN;
    Color albedo{0.5, 0.5, 0.5};
    double emittance_ = 0, shininess = 0, ior = 1;
    static Material diffuse(Color c) { return {RPT_MAT_LAMBERTIAN, c, 0, 0, 1}; }
    static Material specular(Color c, double roughness) { return {RPT_MAT_PHONG, c, 0, roughness, 1}; }
    static Material metallic(Color c, double roughness) { return {RPT_MAT_PHONG, c, 0, roughness, 1}; }
    static Material mirror() { return {RPT_MAT_MIRROR, {0, 0, 0}, 0, 0, 1}; }
    static Material transmissive(double ior) { return {RPT_MAT_TRANSMISSIVE, {0, 0, 0}, 0, 0, ior}; }
    static Material clear(double index, double /*roughness*/) { return {RPT_MAT_TRANSMISSIVE, {0, 0, 0}, 0, 0, index}; }
    static Material transparent(Color c, double index, double /*roughness*/) { return {RPT_MAT_TRANSMISSIVE, c, 0, 0, index}; }
    static Material light(Color c, double emittance) { return {RPT_MAT_LAMBERTIAN, c, emittance, 0, 1}; }
    double emittance() const { return kind <= RPT_MAT_PHONG ? emittance_ : 0.0; }
    Color color() const { return kind <= RPT_MAT_PHONG ? albedo : Color{0, 0, 0}; }
    rpt_material desc() const {
        rpt_material m{};
        m.kind = kind;
        for (int i = 0; i < 3; i++) m.albedo[i] = albedo[i];
        m.emittance = emittance_;
        m.shininess = shininess;
        m.ior = ior;
        return m;
    }
};

// ---- object.rs / light.rs / medium.rs / environment.rs
struct Object {
    Shape shape;
    Material material_;
    explicit Object(Shape s) : shape(std::move(s)) {}
    static Object new_(Shape s) { return Object(std::move(s)); }
    Object material(Material m) && {
        material_ = m;
        return std::move(*this);
    }
    Object material(Material m) const& {
        Object o = *this;
        o.material_ = m;
        return o;
    }
};
struct Light {
    enum Kind { POINT, AMBIENT, DIRECTIONAL, OBJECT } kind;
    Color color{0, 0, 0};
    Vec3 vec{0, 0, 0};
    std::vector<rpt::Object> object;  // 0 or 1 element
    static Light Point(Color c, Vec3 location) { return {POINT, c, location, {}}; }
    static Light Ambient(Color c) { return {AMBIENT, c, {0, 0, 0}, {}}; }
    static Light Directional(Color c, Vec3 direction) { return {DIRECTIONAL, c, direction, {}}; }
    static Light Object(rpt::Object o) { return {OBJECT, {0, 0, 0}, {0, 0, 0}, {std::move(o)}}; }
};
struct Medium {
    int kind;
    double absorption, scattering;
    static Medium homogeneous_isotropic(double a, double s) { return {RPT_MEDIUM_HOMOGENEOUS_ISOTROPIC, a, s}; }
    static Medium colored_glowing_fog(double a, double s) { return {RPT_MEDIUM_COLORED_GLOWING_FOG, a, s}; }
};
struct Environment {  // environment.rs:3-77
    Color color{0, 0, 0};
    uint32_t hdri_width = 0, hdri_height = 0;
    std::vector<double> hdri;  // width*height*3, row-major
    static Environment Color_(Color c) { return {c, 0, 0, {}}; }
    static Environment Hdri(uint32_t width, uint32_t height, std::vector<double> buf) {
        if (buf.size() != size_t(width) * height * 3 || width == 0 || height == 0) throw Error("Hdri::new: bad dimensions");
        return {{0, 0, 0}, width, height, std::move(buf)};
    }
};

// ---- scene.rs
class Scene {
  public:
    std::vector<Object> objects;
    std::vector<Light> lights;
    std::vector<Medium> media;
    Environment environment;
    static Scene new_() { return {}; }
    void add(Object o) { objects.push_back(std::move(o)); }
    void add(Light l) { lights.push_back(std::move(l)); }
    void add(Medium m) { media.push_back(m); }
    // SceneAdd<(Mesh, Material)> / SceneAdd<(Transformed<Cube>, Material)>: object AND light (scene.rs:57-75)
    void add(const std::pair<Shape, Material>& m) {
        bool ok = m.first.kind == RPT_SHAPE_MESH || (m.first.kind == RPT_SHAPE_CUBE && m.first.has_transform);
        if (!ok) throw Error("SceneAdd is implemented for (Mesh, Material) and (Transformed<Cube>, Material)");
        add(Object(m.first).material(m.second));
        add(Light::Object(Object(m.first).material(m.second)));
    }
};

// ---- camera.rs
struct Camera {
    Vec3 eye{0, 0, 10}, direction{0, 0, -1}, up{0, 1, 0};
    double fov = 0.52359877559829887308, aperture = 0, focal_distance = 0;
    static Camera look_at(Vec3 eye, Vec3 center, Vec3 up, double fov) {
        Camera c;
        c.eye = eye;
        c.direction = normalize(center - eye);
        c.up = normalize(up - dot(up, c.direction) * c.direction);
        c.fov = fov;
        return c;
    }
    Camera focus(Vec3 focal_point, double aperture_) const {
        Camera c = *this;
        c.focal_distance = dot(focal_point - eye, direction);
        c.aperture = aperture_;
        return c;
    }
    rpt_camera desc() const {
        rpt_camera c{};
        for (int i = 0; i < 3; i++) {
            c.eye[i] = eye[i];
            c.direction[i] = direction[i];
            c.up[i] = up[i];
        }
        c.fov = fov;
        c.aperture = aperture;
        c.focal_distance = focal_distance;
        return c;
    }
};

// ---- buffer.rs
struct Filter {
    uint32_t radius = 0;
    static Filter Box(uint32_t r) { return {r}; }
};
struct RgbImage {
    uint32_t width = 0, height = 0;
    std::vector<uint8_t> data;  // row-major RGB
};
// buffer.rs:5-97 on the device (rpt_buffer_*): per-pixel running sums; the box filter, color_bytes
// and the variance run where the frame is.
class Buffer {
  public:
    Buffer(uint32_t w, uint32_t h, Filter f, int device = 0) : width(w), height(h), filter(f) {
        h_ = rpt_buffer_create(device, w, h, f.radius);
        if (!h_) throw Error(rpt_last_error());
    }
    Buffer(const Buffer&) = delete;
    Buffer& operator=(const Buffer&) = delete;
    Buffer(Buffer&& o) noexcept : width(o.width), height(o.height), filter(o.filter), h_(o.h_) { o.h_ = nullptr; }
    ~Buffer() {
        if (h_) rpt_buffer_destroy(h_);
    }
    void add_samples(const std::vector<double>& s) {  // buffer.rs:32-40
        if (s.size() != size_t(width) * height * 3) throw Error("Invalid sample dimension");
        if (rpt_buffer_add_samples(h_, s.data()) != RPT_OK) throw Error(rpt_last_error());
    }
    RgbImage image() const {  // buffer.rs:43-56
        RgbImage img{width, height, std::vector<uint8_t>(size_t(width) * height * 3)};
        if (rpt_buffer_image(h_, img.data.data()) != RPT_OK) throw Error(rpt_last_error());
        return img;
    }
    double variance() const {  // buffer.rs:59-73
        double v = 0;
        if (rpt_buffer_variance(h_, &v) != RPT_OK) throw Error(rpt_last_error());
        return v;
    }
    uint32_t batches() const {  // samples[i].len() of the reference (equal for every pixel)
        uint32_t n = 0;
        if (rpt_buffer_batches(h_, &n) != RPT_OK) throw Error(rpt_last_error());
        return n;
    }
    rpt_buffer* raw() const { return h_; }
    // rpt_buffer_mean_device (an addition): per-pixel mean of the batches and the variance of that mean, device pointers
    // (width*height*3 and width*height doubles; d_var may be null).  Needs two batches.
    void mean_device(void* d_rgb, void* d_var, void* hip_stream = nullptr) const {
        if (rpt_buffer_mean_device(h_, d_rgb, d_var, hip_stream) != RPT_OK) throw Error(rpt_last_error());
    }
    // rpt_buffer_denoised_image (an addition): mean -> Denoiser -> color_bytes, no box filter; the feature planes are device pointers.
    RgbImage denoised_image(class Denoiser& denoiser, const rpt_denoise_params& params, const void* d_albedo, const void* d_normal,
                            const void* d_depth) const;
    // rpt_buffer_upsampled_image (an addition): this buffer holds the LOW-resolution batches; mean -> (with a denoiser of this
    // buffer's size: the a-trous filter at the low resolution) -> guided upsampling -> color_bytes.  d_lo[3] / d_hi[3]: the albedo,
    // normal and depth planes of the low and of the full resolution (device pointers, each or null as `params` allows).
    RgbImage upsampled_image(const rpt_upsample_params& params, const void* const d_lo[3], const void* const d_hi[3],
                             class Denoiser* denoiser = nullptr, const rpt_denoise_params* denoise = nullptr) const;
    // Adaptive sampling by tile (rpt_hip.h, an addition).  One batch for the listed 32 x 32 tiles alone (device frame, device list
    // of distinct tile ids), and the batches each tile holds: tiles_x * tiles_y values, row-major.
    void add_samples_tiles_device(const void* d_rgb, const void* d_tiles, uint32_t n_tiles, void* hip_stream = nullptr) {
        if (rpt_buffer_add_samples_tiles_device(h_, d_rgb, d_tiles, n_tiles, hip_stream) != RPT_OK) throw Error(rpt_last_error());
    }
    std::vector<uint32_t> tile_batches() const {
        std::vector<uint32_t> n(size_t((width + 31) / 32) * ((height + 31) / 32));
        if (rpt_buffer_tile_batches(h_, n.data(), n.size()) != RPT_OK) throw Error(rpt_last_error());
        return n;
    }
    // The tiles' errors into d_err (tiles_x * tiles_y doubles on the device); the ids of the tiles still above params.threshold and
    // below params.max_batches into d_tiles_out (ascending) -> their number.
    void tile_errors_device(double floor, void* d_err, void* hip_stream = nullptr) const {
        if (rpt_buffer_tile_errors_device(h_, floor, d_err, hip_stream) != RPT_OK) throw Error(rpt_last_error());
    }
    uint32_t refine_tiles(const rpt_adaptive_params& params, void* d_tiles_out, void* d_err = nullptr, void* hip_stream = nullptr) {
        uint32_t n = 0;
        if (rpt_buffer_refine_tiles(h_, &params, d_tiles_out, &n, d_err, hip_stream) != RPT_OK) throw Error(rpt_last_error());
        return n;
    }
    uint32_t width, height;
    Filter filter;

  private:
    rpt_buffer* h_ = nullptr;
};
// The a-trous denoiser of rpt_hip.h (rpt_denoise*, an addition): owns the scratch of one frame size on one device.
class Denoiser {
  public:
    // passes 4, demodulation and id match on, sigma_color 4, sigma_normal 0.5, depth term off (it is in scene units per pixel step)
    static rpt_denoise_params default_params() { return {4, RPT_DENOISE_DEMODULATE | RPT_DENOISE_MATCH_ID, 4.0, 0.5, 0.0}; }
    Denoiser(uint32_t w, uint32_t h, int device = 0) : width(w), height(h) {
        h_ = rpt_denoiser_create(device, w, h);
        if (!h_) throw Error(rpt_last_error());
    }
    Denoiser(const Denoiser&) = delete;
    Denoiser& operator=(const Denoiser&) = delete;
    Denoiser(Denoiser&& o) noexcept : width(o.width), height(o.height), h_(o.h_) { o.h_ = nullptr; }
    ~Denoiser() {
        if (h_) rpt_denoiser_destroy(h_);
    }
    // host arrays: rgb, albedo, normal, depth of width*height*3 doubles, var of width*height; an empty vector is a null plane
    std::vector<double> denoise(const rpt_denoise_params& params, const std::vector<double>& rgb, const std::vector<double>& var,
                                const std::vector<double>& albedo, const std::vector<double>& normal, const std::vector<double>& depth,
                                std::vector<double>* out_var = nullptr) {
        const size_t n = size_t(width) * height;
        auto ptr = [&](const std::vector<double>& v, size_t want) -> const double* {
            if (v.empty()) return nullptr;
            if (v.size() != want) throw Error("Invalid plane dimension");
            return v.data();
        };
        std::vector<double> out(n * 3);
        if (out_var) out_var->assign(n, 0.0);
        if (rpt_denoise(h_, &params, ptr(rgb, n * 3), ptr(var, n), ptr(albedo, n * 3), ptr(normal, n * 3), ptr(depth, n * 3), out.data(),
                        out_var ? out_var->data() : nullptr) != RPT_OK)
            throw Error(rpt_last_error());
        return out;
    }
    void denoise_device(const rpt_denoise_params& params, const void* d_rgb, const void* d_var, const void* d_albedo, const void* d_normal,
                        const void* d_depth, void* d_out, void* d_out_var = nullptr, void* hip_stream = nullptr) {
        if (rpt_denoise_device(h_, &params, d_rgb, d_var, d_albedo, d_normal, d_depth, d_out, d_out_var, hip_stream) != RPT_OK)
            throw Error(rpt_last_error());
    }
    rpt_denoiser* raw() const { return h_; }
    uint32_t width, height;

  private:
    rpt_denoiser* h_ = nullptr;
};
inline RgbImage Buffer::denoised_image(Denoiser& denoiser, const rpt_denoise_params& params, const void* d_albedo, const void* d_normal,
                                       const void* d_depth) const {
    RgbImage img{width, height, std::vector<uint8_t>(size_t(width) * height * 3)};
    if (rpt_buffer_denoised_image(h_, denoiser.raw(), &params, d_albedo, d_normal, d_depth, img.data.data()) != RPT_OK) throw Error(rpt_last_error());
    return img;
}
inline RgbImage Buffer::upsampled_image(const rpt_upsample_params& params, const void* const d_lo[3], const void* const d_hi[3], Denoiser* denoiser,
                                        const rpt_denoise_params* denoise) const {
    const uint32_t s = params.scale >= 2 && params.scale <= 4 ? params.scale : 1;   // (a bad scale: the call below refuses it)
    RgbImage img{width * s, height * s, std::vector<uint8_t>(size_t(width) * s * height * s * 3)};
    const rpt_denoise_params dflt = Denoiser::default_params();
    if (rpt_buffer_upsampled_image(h_, denoiser ? denoiser->raw() : nullptr, denoise ? denoise : &dflt, &params, d_lo[0], d_lo[1], d_lo[2], d_hi[0],
                                   d_hi[1], d_hi[2], img.data.data()) != RPT_OK)
        throw Error(rpt_last_error());
    return img;
}
// Guided upsampling (rpt_upsample*, an addition): a frame rendered at (w, h) and its variance taken to (s w, s h) under the feature
// planes of both sizes.  Stateless: thin wrappers of the C entry points.
struct Upsample {
    // s = 2, bilinear 2 x 2 taps, demodulation and id match on, sigma_normal 1 ("Guided upsampling"), depth term
    // off (it is in scene units per low-resolution pixel)
    static rpt_upsample_params default_params() { return {2, 1, RPT_UPSAMPLE_DEMODULATE | RPT_UPSAMPLE_MATCH_ID, 0, 1.0, 0.0}; }
    // device pointers on the current device; d_lo[3] / d_hi[3]: albedo, normal, depth, each or null as `params` allows
    static void run_device(const rpt_upsample_params& params, uint32_t lo_width, uint32_t lo_height, const void* d_lo_rgb, const void* d_lo_var,
                           const void* const d_lo[3], const void* const d_hi[3], void* d_out, void* d_out_var = nullptr, void* hip_stream = nullptr) {
        if (rpt_upsample_device(&params, lo_width, lo_height, d_lo_rgb, d_lo_var, d_lo[0], d_lo[1], d_lo[2], d_hi[0], d_hi[1], d_hi[2], d_out, d_out_var,
                                hip_stream) != RPT_OK)
            throw Error(rpt_last_error());
    }
    // host arrays; an empty vector is a null plane
    static std::vector<double> run(const rpt_upsample_params& params, uint32_t lo_width, uint32_t lo_height, const std::vector<double>& lo_rgb,
                                   const std::vector<double>& lo_var, const std::vector<double> (&lo)[3], const std::vector<double> (&hi)[3],
                                   std::vector<double>* out_var = nullptr, int device = 0) {
        if (params.scale < 2 || params.scale > 4) throw Error("scale must be 2, 3 or 4");   // (before anything is sized by it)
        const uint64_t W = uint64_t(lo_width) * params.scale, H = uint64_t(lo_height) * params.scale;
        if (W >= (1ull << 32) || H >= (1ull << 32) || W * H >= (1ull << 31)) throw Error("the full-resolution frame is too large");
        const size_t n = size_t(lo_width) * lo_height, N = n * params.scale * params.scale;
        auto ptr = [&](const std::vector<double>& v, size_t want) -> const double* {
            if (v.empty()) return nullptr;
            if (v.size() != want) throw Error("Invalid plane dimension");
            return v.data();
        };
        std::vector<double> out(N * 3);
        if (out_var) out_var->assign(N, 0.0);
        if (rpt_upsample(device, &params, lo_width, lo_height, ptr(lo_rgb, n * 3), ptr(lo_var, n), ptr(lo[0], n * 3), ptr(lo[1], n * 3), ptr(lo[2], n * 3),
                         ptr(hi[0], N * 3), ptr(hi[1], N * 3), ptr(hi[2], N * 3), out.data(), out_var ? out_var->data() : nullptr) != RPT_OK)
            throw Error(rpt_last_error());
        return out;
    }
    // rpt_image_bytes_device: color_bytes of a device plane, only the bytes come back
    static RgbImage image_bytes_device(const void* d_rgb, uint32_t width, uint32_t height, void* hip_stream = nullptr) {
        if (uint64_t(width) * height >= (1ull << 31)) throw Error("bad image size");   // (before anything is sized by it)
        RgbImage img{width, height, std::vector<uint8_t>(size_t(width) * height * 3)};
        if (rpt_image_bytes_device(d_rgb, width, height, img.data.data(), hip_stream) != RPT_OK) throw Error(rpt_last_error());
        return img;
    }
};
// Temporal accumulation with reprojection (rpt_temporal_*, an addition): owns the history of a frame sequence of one size on one
// device.  For a camera that moves over a scene whose objects keep their places and indices.
class Temporal {
  public:
    // history of 16 frames, id match on, depth_tol 0.1 (relative, on squared distances), normal_tol 0.5
    static rpt_temporal_params default_params() { return {16, RPT_TEMPORAL_MATCH_ID, 0.1, 0.5}; }
    // eye, direction, right, up, d: what the accumulation takes of a camera (a host function)
    static std::array<double, 13> camera_record(const Camera& camera) {
        std::array<double, 13> r{};
        const rpt_camera c = camera.desc();
        if (rpt_temporal_camera_record(&c, r.data()) != RPT_OK) throw Error(rpt_last_error());
        return r;
    }
    // A (3 x 4), G (3 x 3), three zeros: the motion record of an object whose composed object-to-world matrices (row-major 4 x 4)
    // are `cur` in the current and `prev` in the previous frame (a host function)
    static std::array<double, RPT_TEMPORAL_MOTION_DOUBLES> motion_record(const std::array<double, 16>& cur, const std::array<double, 16>& prev) {
        std::array<double, RPT_TEMPORAL_MOTION_DOUBLES> r{};
        if (rpt_temporal_motion_record(cur.data(), prev.data(), r.data()) != RPT_OK) throw Error(rpt_last_error());
        return r;
    }
    // the one-shot motion table of the next accumulate / accumulate_device / frame_image: record i for the object with id i + 1
    // (copied; an empty vector clears it)
    void set_motion(const std::vector<std::array<double, RPT_TEMPORAL_MOTION_DOUBLES>>& records) {
        if (rpt_temporal_set_motion(h_, records.empty() ? nullptr : records[0].data(), uint32_t(records.size())) != RPT_OK) throw Error(rpt_last_error());
    }
    // ... as a device table that the caller owns and leaves unchanged until the consuming call's work is done
    void set_motion_device(const void* d_records, uint32_t n_objects) {
        if (rpt_temporal_set_motion_device(h_, d_records, n_objects) != RPT_OK) throw Error(rpt_last_error());
    }
    // the settings of RPT_TEMPORAL_CLIP (params.flags): window radius 1..3, gamma >= 0, the history length a clipped pixel keeps
    // (0: all of it); they persist over calls and resets
    void set_clip(uint32_t radius = 1, double gamma = 0.5, uint32_t clip_history = 1) {
        if (rpt_temporal_set_clip(h_, radius, gamma, clip_history) != RPT_OK) throw Error(rpt_last_error());
    }
    Temporal(uint32_t w, uint32_t h, int device = 0) : width(w), height(h) {
        h_ = rpt_temporal_create(device, w, h);
        if (!h_) throw Error(rpt_last_error());
    }
    Temporal(const Temporal&) = delete;
    Temporal& operator=(const Temporal&) = delete;
    Temporal(Temporal&& o) noexcept : width(o.width), height(o.height), h_(o.h_) { o.h_ = nullptr; }
    ~Temporal() {
        if (h_) rpt_temporal_destroy(h_);
    }
    // host arrays: rgb, normal, depth of width*height*3 doubles, var of width*height; an empty vector is a null plane (normal is
    // empty iff params.normal_tol == 0) -> the accumulated frame; its variance and the history lengths where asked for
    std::vector<double> accumulate(const rpt_temporal_params& params, const Camera& camera, const std::vector<double>& rgb,
                                   const std::vector<double>& var, const std::vector<double>& normal, const std::vector<double>& depth,
                                   std::vector<double>* out_var = nullptr, std::vector<double>* out_len = nullptr) {
        const size_t n = size_t(width) * height;
        auto ptr = [&](const std::vector<double>& v, size_t want) -> const double* {
            if (v.empty()) return nullptr;
            if (v.size() != want) throw Error("Invalid plane dimension");
            return v.data();
        };
        std::vector<double> out(n * 3);
        if (out_var) out_var->assign(n, 0.0);
        if (out_len) out_len->assign(n, 0.0);
        const rpt_camera c = camera.desc();
        if (rpt_temporal_accumulate(h_, &params, &c, ptr(rgb, n * 3), ptr(var, n), ptr(normal, n * 3), ptr(depth, n * 3), out.data(),
                                    out_var ? out_var->data() : nullptr, out_len ? out_len->data() : nullptr) != RPT_OK)
            throw Error(rpt_last_error());
        return out;
    }
    void accumulate_device(const rpt_temporal_params& params, const Camera& camera, const void* d_rgb, const void* d_var, const void* d_normal,
                           const void* d_depth, void* d_out, void* d_out_var = nullptr, void* d_out_len = nullptr, void* hip_stream = nullptr) {
        const rpt_camera c = camera.desc();
        if (rpt_temporal_accumulate_device(h_, &params, &c, d_rgb, d_var, d_normal, d_depth, d_out, d_out_var, d_out_len, hip_stream) != RPT_OK)
            throw Error(rpt_last_error());
    }
    // rpt_temporal_preview_device: what accumulate_device would write in the listed 32 x 32 tiles (d_tiles: a device list of n_tiles
    // distinct ids; nullptr with 0: every tile); nothing of the accumulator changes and a pending motion table stays set.
    void preview_device(const rpt_temporal_params& params, const Camera& camera, const void* d_rgb, const void* d_var, const void* d_normal,
                        const void* d_depth, const void* d_tiles, uint32_t n_tiles, void* d_out, void* d_out_var = nullptr, void* d_out_len = nullptr,
                        void* hip_stream = nullptr) {
        const rpt_camera c = camera.desc();
        if (rpt_temporal_preview_device(h_, &params, &c, d_rgb, d_var, d_normal, d_depth, d_tiles, n_tiles, d_out, d_out_var, d_out_len, hip_stream) != RPT_OK)
            throw Error(rpt_last_error());
    }
    // rpt_temporal_tile_errors_device: Buffer::tile_errors_device's error of the listed tiles with the pixel's terms taken from planes
    void tile_errors_device(const void* d_rgb, const void* d_var, double floor, const void* d_tiles, uint32_t n_tiles, void* d_err,
                            void* hip_stream = nullptr) const {
        if (rpt_temporal_tile_errors_device(h_, d_rgb, d_var, floor, d_tiles, n_tiles, d_err, hip_stream) != RPT_OK) throw Error(rpt_last_error());
    }
    // rpt_temporal_frame_image: the buffer's mean and variance -> accumulate -> (with a denoiser: the a-trous filter with the
    // accumulated variance) -> color_bytes; the feature planes are device pointers.
    RgbImage frame_image(const rpt_temporal_params& params, const Camera& camera, const Buffer& buffer, const void* d_albedo,
                         const void* d_normal, const void* d_depth, Denoiser* denoiser = nullptr,
                         const rpt_denoise_params& denoise = Denoiser::default_params()) {
        RgbImage img{width, height, std::vector<uint8_t>(size_t(width) * height * 3)};
        const rpt_camera c = camera.desc();
        if (rpt_temporal_frame_image(h_, &params, &c, buffer.raw(), denoiser ? denoiser->raw() : nullptr, &denoise, d_albedo, d_normal, d_depth,
                                     img.data.data()) != RPT_OK)
            throw Error(rpt_last_error());
        return img;
    }
    void reset() {  // forget the history
        if (rpt_temporal_reset(h_) != RPT_OK) throw Error(rpt_last_error());
    }
    uint32_t frames() const {  // since the creation or the last reset
        uint32_t n = 0;
        if (rpt_temporal_frames(h_, &n) != RPT_OK) throw Error(rpt_last_error());
        return n;
    }
    rpt_temporal* raw() const { return h_; }
    uint32_t width, height;

  private:
    rpt_temporal* h_ = nullptr;
};

// ---- renderer.rs
class Renderer {
  public:
    Renderer(const Scene& scene, Camera camera) : scene_(scene), camera_(camera) {}
    static Renderer new_(const Scene& scene, Camera camera) { return Renderer(scene, camera); }
    Renderer(const Renderer&) = delete;
    Renderer(Renderer&& o) noexcept : scene_(o.scene_), camera_(o.camera_), p_(o.p_), handle_(o.handle_) { o.handle_ = nullptr; }
    ~Renderer() {
        if (handle_) rpt_scene_destroy(handle_);
    }
    struct Params {
        uint32_t width = 800, height = 600;
        double exposure_value = 0, stepsize = 0;
        Filter filter;
        uint32_t max_bounces = 0, num_samples = 1;
        size_t gather_size = 50, gather_size_volume = 50;
        double watts = 100;
        uint64_t seed = 0;                   // addition: the reference seeds from entropy (renderer.rs:163)
        uint32_t shard_rank = 0, shard_count = 1;
        int device = 0;
    };
#define RPT_BUILDER(name, type) \
    Renderer&& name(type v) && { p_.name = v; return std::move(*this); } \
    Renderer& name(type v) & { p_.name = v; return *this; }
    RPT_BUILDER(width, uint32_t)
    RPT_BUILDER(height, uint32_t)
    RPT_BUILDER(exposure_value, double)
    RPT_BUILDER(stepsize, double)
    RPT_BUILDER(filter, Filter)
    RPT_BUILDER(max_bounces, uint32_t)
    RPT_BUILDER(num_samples, uint32_t)
    RPT_BUILDER(gather_size, size_t)
    RPT_BUILDER(gather_size_volume, size_t)
    RPT_BUILDER(watts, double)
    RPT_BUILDER(seed, uint64_t)
    RPT_BUILDER(device, int)
#undef RPT_BUILDER
    Renderer& shard(uint32_t rank, uint32_t count) {
        p_.shard_rank = rank;
        p_.shard_count = count;
        return *this;
    }
    const Params& params() const { return p_; }

    RgbImage render() {  // renderer.rs:137-141
        Buffer buffer(p_.width, p_.height, p_.filter, p_.device);
        sample_offset_ = 0;
        sample(p_.num_samples, buffer);
        return buffer.image();
    }
    void iterative_render(uint32_t callback_interval, const std::function<void(uint32_t, const Buffer&)>& cb) {
        Buffer buffer(p_.width, p_.height, p_.filter, p_.device);  // renderer.rs:144-156
        sample_offset_ = 0;
        uint32_t iteration = 0;
        while (iteration < p_.num_samples) {
            uint32_t steps = std::min(p_.num_samples - iteration, callback_interval);
            sample(steps, buffer);
            iteration += steps;
            cb(iteration, buffer);
        }
    }
    // ---- photon mapping (photon.rs:631-720)
    enum PhotonRenderKind { PhotonMap = RPT_PHOTON_MAP, PhotonPointBeam = RPT_PHOTON_POINT_BEAM, PhotonBeamBeam = RPT_PHOTON_BEAM_BEAM };
    RgbImage photon_render(size_t photon_count, PhotonRenderKind kind) {  // photon.rs:655-720
        commit();
        check(rpt_photon_map_build(handle_, photon_count, int32_t(kind), p_.watts, p_.seed));
        Buffer buffer(p_.width, p_.height, p_.filter, p_.device);
        std::vector<double> out(size_t(p_.width) * p_.height * 3);
        rpt_camera cam = camera_.desc();
        rpt_render_params rp{p_.width, p_.height, p_.exposure_value, p_.max_bounces, p_.shard_rank, p_.shard_count};
        check(rpt_photon_render_sample(handle_, &cam, &rp, p_.gather_size, p_.gather_size_volume, p_.num_samples, p_.seed, 0,
                                       out.data()));
        buffer.add_samples(out);
        return buffer.image();
    }
    RgbImage photon_point_query_beam_render(size_t n) { return photon_render(n, PhotonPointBeam); }  // :642-644
    RgbImage photon_beam_query_beam_render(size_t n) { return photon_render(n, PhotonBeamBeam); }   // :646-648
    RgbImage photon_map_render(size_t n) { return photon_render(n, PhotonMap); }                     // :650-652

    // One batch of a multi-GPU render: this rank's tiles into the device frame d_frame
    // (width * height * 3 f64 on this renderer's device), then the gather of every rank's tiles onto rank 0, all
    // enqueued on hip_stream.  shard(rank, count) must match the communicator.
    void sample_sharded(uint32_t iterations, class Comm& comm, void* d_frame, void* hip_stream = nullptr);

    // Renderer::sample (renderer.rs:158-171): the call that crosses the C ABI.
    void sample(uint32_t iterations, Buffer& buffer) {  // renderer.rs:158-171; the batch stays on the device
        commit();
        rpt_camera cam = camera_.desc();
        rpt_render_params rp{p_.width, p_.height, p_.exposure_value, p_.max_bounces, p_.shard_rank, p_.shard_count};
        check(rpt_render_into_buffer(handle_, &cam, &rp, iterations, p_.seed, sample_offset_, buffer.raw()));
        sample_offset_ += iterations;
    }

    // Tile-list renders (rpt_hip.h, an addition): `iterations` samples of the listed 32 x 32 tiles alone, the bits sample() would
    // put there; every other element of the frame is left as it is.  Not sharded.  The sample offset advances as in sample().
    void sample_tiles_device(uint32_t iterations, const void* d_tiles, uint32_t n_tiles, void* d_frame, void* hip_stream = nullptr) {
        commit();
        rpt_camera cam = camera_.desc();
        rpt_render_params rp{p_.width, p_.height, p_.exposure_value, p_.max_bounces, p_.shard_rank, p_.shard_count};
        check(rpt_render_sample_tiles_device(handle_, &cam, &rp, iterations, p_.seed, sample_offset_, d_tiles, n_tiles, d_frame, hip_stream));
        sample_offset_ += iterations;
    }
    void sample_tiles(uint32_t iterations, const std::vector<uint32_t>& tiles, std::vector<double>& frame) {
        if (frame.size() != size_t(p_.width) * p_.height * 3) throw Error("Invalid sample dimension");
        commit();
        rpt_camera cam = camera_.desc();
        rpt_render_params rp{p_.width, p_.height, p_.exposure_value, p_.max_bounces, p_.shard_rank, p_.shard_count};
        check(rpt_render_sample_tiles(handle_, &cam, &rp, iterations, p_.seed, sample_offset_, tiles.data(), uint32_t(tiles.size()), frame.data()));
        sample_offset_ += iterations;
    }
    // rpt_render_adaptive: min_batches full frames, then tile lists while a tile's error is above the threshold, into an empty buffer
    // -> rounds, tile-batches rendered, tiles at max_batches, tiles.
    static rpt_adaptive_params default_adaptive_params() { return {4, 4, 16, 0, 0.05, 0.05}; }
    std::array<uint64_t, 4> render_adaptive(const rpt_adaptive_params& params, Buffer& buffer) {
        commit();
        rpt_camera cam = camera_.desc();
        rpt_render_params rp{p_.width, p_.height, p_.exposure_value, p_.max_bounces, p_.shard_rank, p_.shard_count};
        std::array<uint64_t, 4> stats{};
        check(rpt_render_adaptive(handle_, &cam, &rp, &params, p_.seed, buffer.raw(), stats.data()));
        return stats;
    }
    // rpt_render_adaptive_temporal: render_adaptive with a tile's error taken from the preview of `temporal`'s accumulation of the frame
    // so far, batch k at sample_offset + k spp_per_batch; nothing is accumulated (Temporal::frame_image finishes the frame).
    std::array<uint64_t, 4> render_adaptive_temporal(const rpt_adaptive_params& params, Buffer& buffer, Temporal& temporal,
                                                     const rpt_temporal_params& temporal_params, const void* d_normal, const void* d_depth,
                                                     uint32_t sample_offset = 0) {
        commit();
        rpt_camera cam = camera_.desc();
        rpt_render_params rp{p_.width, p_.height, p_.exposure_value, p_.max_bounces, p_.shard_rank, p_.shard_count};
        std::array<uint64_t, 4> stats{};
        check(rpt_render_adaptive_temporal(handle_, &cam, &rp, &params, p_.seed, sample_offset, buffer.raw(), temporal.raw(), &temporal_params, d_normal,
                                           d_depth, stats.data()));
        return stats;
    }

    // First-hit feature planes (rpt_hip.h, rpt_render_features: an addition) of the camera samples the next sample() call traces --
    // same seed, same sample offset, which is not advanced --: width * height * 3 doubles each, the frame's own layout.
    struct Features {
        std::vector<double> albedo;   // mean Material::color of the first hit, the environment's colour on a miss
        std::vector<double> normal;   // mean normal (0 on a miss), not renormalised
        std::vector<double> depth;    // (mean hit distance over all samples, coverage, object index + 1 of the first sample or 0)
    };
    Features features(uint32_t iterations) {
        commit();
        const size_t n = size_t(p_.width) * p_.height * 3;
        Features f{std::vector<double>(n), std::vector<double>(n), std::vector<double>(n)};
        rpt_camera cam = camera_.desc();
        rpt_render_params rp{p_.width, p_.height, p_.exposure_value, p_.max_bounces, p_.shard_rank, p_.shard_count};
        check(rpt_render_features(handle_, &cam, &rp, iterations, p_.seed, sample_offset_, f.albedo.data(), f.normal.data(), f.depth.data()));
        return f;
    }
    // ... into device planes on this renderer's device (null: not computed), enqueued on hip_stream.
    void features_device(uint32_t iterations, void* d_albedo, void* d_normal, void* d_depth, void* hip_stream = nullptr) {
        commit();
        rpt_camera cam = camera_.desc();
        rpt_render_params rp{p_.width, p_.height, p_.exposure_value, p_.max_bounces, p_.shard_rank, p_.shard_count};
        check(rpt_render_features_device(handle_, &cam, &rp, iterations, p_.seed, sample_offset_, d_albedo, d_normal, d_depth, hip_stream));
    }

    // The candidate trees of the reference-epsilon mode's large meshes (rpt_hip.h, rpt_f64_mesh_tree_info): meshes, triangles, nodes,
    // depth, bytes, render uses the trees, photon passes use them, threshold.  Throws for a scene of the fp32 path.
    std::array<uint64_t, 8> f64_mesh_tree_info() {
        commit();
        std::array<uint64_t, 8> out{};
        check(rpt_f64_mesh_tree_info(handle_, out.data()));
        return out;
    }

    // Moving spheres (rpt_hip.h, rpt_scene_set_movable_spheres; the committed scene is this renderer's, so the calls live here and not in
    // Scene, which stays a description): `objects` are indices into scene.objects of spheres under translate(c) * scale(r, r, r).
    // move_spheres: host centres (and offsets added to them, or none), synchronous; returns the motion table (scene.objects.size()
    // x 24 doubles, identity for the objects that are not listed) when asked for one.  move_spheres_device: centres, offsets and
    // motion table in device memory, asynchronous on hip_stream and ordered like a render of the scene.
    void set_movable_spheres(const std::vector<uint32_t>& objects) {
        commit();
        check(rpt_scene_set_movable_spheres(handle_, objects.data(), uint32_t(objects.size())));
    }
    std::vector<double> move_spheres(const std::vector<Vec3>& centres, const std::vector<Vec3>* offsets = nullptr, bool motion = false) {
        commit();
        std::array<uint64_t, 8> info{};
        check(rpt_scene_movable_info(handle_, info.data()));
        if (centres.size() != info[1] || (offsets && offsets->size() != info[1])) throw Error("move_spheres: one centre (and offset) per movable sphere");
        std::vector<double> table(motion ? scene_.objects.size() * 24 : 0);
        check(rpt_scene_move_spheres(handle_, centres.empty() ? nullptr : centres[0].data(), offsets && !offsets->empty() ? (*offsets)[0].data() : nullptr,
                                     motion ? table.data() : nullptr));
        return table;
    }
    void move_spheres_device(const void* d_centres, const void* d_offsets = nullptr, void* d_motion = nullptr, void* hip_stream = nullptr) {
        commit();
        check(rpt_scene_move_spheres_device(handle_, d_centres, d_offsets, d_motion, hip_stream));
    }

  private:
    void commit() {
        if (handle_) return;
        rpt_scene* h = rpt_scene_create();
        try {
            for (const Object& o : scene_.objects) {
                rpt_shape_desc d = o.shape.desc();
                rpt_material m = o.material_.desc();
                check(rpt_scene_add_object(h, &d, &m));
            }
            for (const Light& l : scene_.lights) {
                switch (l.kind) {
                    case Light::POINT: check(rpt_scene_add_light_point(h, l.color.data(), l.vec.data())); break;
                    case Light::AMBIENT: check(rpt_scene_add_light_ambient(h, l.color.data())); break;
                    case Light::DIRECTIONAL: check(rpt_scene_add_light_directional(h, l.color.data(), l.vec.data())); break;
                    default: {
                        rpt_shape_desc d = l.object.at(0).shape.desc();
                        rpt_material m = l.object.at(0).material_.desc();
                        check(rpt_scene_add_light_object(h, &d, &m));
                    }
                }
            }
            for (const Medium& m : scene_.media) check(rpt_scene_add_medium(h, m.kind, m.absorption, m.scattering));
            if (scene_.environment.hdri_width)
                check(rpt_scene_set_environment_hdri(h, scene_.environment.hdri_width, scene_.environment.hdri_height,
                                                     scene_.environment.hdri.data()));
            else
                check(rpt_scene_set_environment_color(h, scene_.environment.color.data()));
            check(rpt_scene_commit(h, p_.device));
        } catch (...) {
            rpt_scene_destroy(h);
            throw;
        }
        handle_ = h;
    }
    const Scene& scene_;
    Camera camera_;
    Params p_;
    rpt_scene* handle_ = nullptr;
    uint32_t sample_offset_ = 0;
};

// The frame exchange between the GPUs of one node (rpt_comm_*, rpt_gather_frame_device): one process per GPU, rank 0
// assembles the image from the tiles every rank owns.  Rank 0 draws the id (Comm::unique_id) and hands its 128 bytes to
// the other ranks by whatever means the launcher offers.
class Comm {
  public:
    using Id = std::array<unsigned char, RPT_COMM_ID_BYTES>;
    static Id unique_id() {
        Id id{};
        check(rpt_comm_unique_id(id.data()));
        return id;
    }
    Comm(const Id& id, int rank, int n_ranks, int device) { check(rpt_comm_create(id.data(), rank, n_ranks, device, &h_)); }
    Comm(const Comm&) = delete;
    Comm& operator=(const Comm&) = delete;
    ~Comm() { rpt_comm_destroy(h_); }
    int rank() const { int r = 0; check(rpt_comm_rank(h_, &r, nullptr)); return r; }
    int size() const { int n = 0; check(rpt_comm_rank(h_, nullptr, &n)); return n; }
    // Collective: d_shard = this rank's frame, d_frame = where rank 0 assembles (may be d_shard; ignored elsewhere).
    void gather(uint32_t width, uint32_t height, const void* d_shard, void* d_frame, void* hip_stream = nullptr, bool loopback = false) {
        check(rpt_gather_frame_device(h_, width, height, d_shard, d_frame, loopback ? RPT_GATHER_LOOPBACK : 0u, hip_stream));
    }
    rpt_comm* raw() const { return h_; }

  private:
    rpt_comm* h_ = nullptr;
};
inline void Renderer::sample_sharded(uint32_t iterations, Comm& comm, void* d_frame, void* hip_stream) {
    commit();
    rpt_camera cam = camera_.desc();
    rpt_render_params rp{p_.width, p_.height, p_.exposure_value, p_.max_bounces, p_.shard_rank, p_.shard_count};
    check(rpt_render_sample_device(handle_, &cam, &rp, iterations, p_.seed, sample_offset_, d_frame, hip_stream));
    sample_offset_ += iterations;
    comm.gather(p_.width, p_.height, d_frame, d_frame, hip_stream);
}

// ---- src/ode/: ParticleState, the ParticleSystem trait and its three systems (rpt_particles_*; rpt_hip.h states the arithmetic).
struct ParticleState {
    std::vector<Vec3> pos, vel;
    size_t size() const { return pos.size(); }
};
inline ParticleState operator+(const ParticleState& a, const ParticleState& b) {
    ParticleState r = a;
    for (size_t i = 0; i < r.pos.size(); i++)
        for (int k = 0; k < 3; k++) {
            r.pos[i][k] = a.pos[i][k] + b.pos[i][k];
            r.vel[i][k] = a.vel[i][k] + b.vel[i][k];
        }
    return r;
}
inline ParticleState operator*(const ParticleState& a, double f) {
    ParticleState r = a;
    for (size_t i = 0; i < r.pos.size(); i++)
        for (int k = 0; k < 3; k++) {
            r.pos[i][k] = a.pos[i][k] * f;
            r.vel[i][k] = a.vel[i][k] * f;
        }
    return r;
}
inline ParticleState operator/(const ParticleState& a, double f) {
    ParticleState r = a;
    for (size_t i = 0; i < r.pos.size(); i++)
        for (int k = 0; k < 3; k++) {
            r.pos[i][k] = a.pos[i][k] / f;
            r.vel[i][k] = a.vel[i][k] / f;
        }
    return r;
}
// The open trait: a system of the caller's own overrides time_derivative and integrates on the host, with the operation order of
// rpt_hip.h (k1 .. k4, ((k1 + k2 2) + k3 2) + k4, the reference's time loop).  Compile without fp contraction to get its bits.
class ParticleSystem {
  public:
    virtual ~ParticleSystem() = default;
    virtual ParticleState time_derivative(const ParticleState& state) const = 0;
    virtual void rk4_integrate(ParticleState& state, double time, double step) const {
        auto one = [&](double h) {
            const ParticleState k1 = time_derivative(state);
            const ParticleState k2 = time_derivative(state + k1 * (h / 2.0));
            const ParticleState k3 = time_derivative(state + k2 * (h / 2.0));
            const ParticleState k4 = time_derivative(state + k3 * h);
            state = state + (((k1 + k2 * 2.0) + k3 * 2.0) + k4) * (h / 6.0);
        };
        while (time > step) {
            one(step);
            time = time - step;
        }
        one(time);
    }
};
// A system's state on a device (rpt_particles): the calls of one simulator are ordered whatever their streams.
class ParticleSimulator {
  public:
    ParticleSimulator(const rpt_particles_params& prm, const ParticleState& state, int device = 0) : n_(prm.n) {
        h_ = rpt_particles_create(device, &prm);
        if (!h_) throw Error(rpt_last_error());
        set_state(state);
    }
    ParticleSimulator(const ParticleSimulator&) = delete;
    ParticleSimulator& operator=(const ParticleSimulator&) = delete;
    ~ParticleSimulator() { rpt_particles_destroy(h_); }
    void set_state(const ParticleState& s) {
        if (s.pos.size() != n_ || s.vel.size() != n_) throw Error("ParticleSimulator: the state has another number of particles");
        check(rpt_particles_set_state(h_, s.pos[0].data(), s.vel[0].data()));   // (std::array<double, 3>: n x 3 contiguous doubles)
    }
    ParticleState state() const {
        ParticleState s{std::vector<Vec3>(n_), std::vector<Vec3>(n_)};
        check(rpt_particles_state(h_, s.pos[0].data(), s.vel[0].data()));
        return s;
    }
    void integrate(double time, double step, void* hip_stream = nullptr) { check(rpt_particles_integrate(h_, time, step, hip_stream)); }
    std::vector<Vec3> display_positions() const {
        std::vector<Vec3> out(n_);
        check(rpt_particles_display_positions(h_, out[0].data()));
        return out;
    }
    // The same positions left in the simulator's own device array (n x 3 doubles): asynchronous, ordered like integrate.
    void* display_positions_device(void* hip_stream = nullptr) const {
        void* d = nullptr;
        check(rpt_particles_display_positions_device(h_, &d, hip_stream));
        return d;
    }
    std::array<uint64_t, 8> counters() const {
        std::array<uint64_t, 8> c{};
        check(rpt_particles_counters(h_, c.data()));
        return c;
    }
    rpt_particles* raw() const { return h_; }

  private:
    rpt_particles* h_ = nullptr;
    uint32_t n_ = 0;
};
// Many independent systems on a device, integrated in one launch (rpt_particles_batch): system i of `prm` with state i of `states`.
// Every system comes out with the bits it would have alone; the calls of one ensemble are ordered whatever their streams.
class ParticleEnsemble {
  public:
    ParticleEnsemble(const std::vector<rpt_particles_params>& prm, const std::vector<ParticleState>& states, int device = 0) {
        if (prm.size() != states.size()) throw Error("ParticleEnsemble: as many states as systems");
        first_.push_back(0);
        for (size_t i = 0; i < prm.size(); i++) {
            if (states[i].pos.size() != prm[i].n || states[i].vel.size() != prm[i].n) throw Error("ParticleEnsemble: a state has another number of particles");
            first_.push_back(first_.back() + prm[i].n);
        }
        h_ = rpt_particles_batch_create(device, prm.data(), uint32_t(prm.size()));
        if (!h_) throw Error(rpt_last_error());
        std::vector<Vec3> pos, vel;
        for (const ParticleState& s : states) {
            pos.insert(pos.end(), s.pos.begin(), s.pos.end());
            vel.insert(vel.end(), s.vel.begin(), s.vel.end());
        }
        const int rc = rpt_particles_batch_set_state(h_, pos[0].data(), vel[0].data());
        if (rc != RPT_OK) {
            rpt_particles_batch_destroy(h_);
            check(rc);
        }
    }
    ParticleEnsemble(const ParticleEnsemble&) = delete;
    ParticleEnsemble& operator=(const ParticleEnsemble&) = delete;
    ~ParticleEnsemble() { rpt_particles_batch_destroy(h_); }
    size_t size() const { return first_.size() - 1; }
    void set_state(size_t i, const ParticleState& s) {
        if (i >= size()) throw Error("ParticleEnsemble: system index out of range");
        if (s.pos.size() != first_[i + 1] - first_[i] || s.vel.size() != s.pos.size()) throw Error("ParticleEnsemble: the state has another number of particles");
        check(rpt_particles_batch_set_system_state(h_, uint32_t(i), s.pos[0].data(), s.vel[0].data()));
    }
    std::vector<ParticleState> states() const {
        std::vector<Vec3> pos(first_.back()), vel(first_.back());
        check(rpt_particles_batch_state(h_, pos[0].data(), vel[0].data()));
        std::vector<ParticleState> out;
        for (size_t i = 0; i < size(); i++)
            out.push_back({std::vector<Vec3>(pos.begin() + first_[i], pos.begin() + first_[i + 1]), std::vector<Vec3>(vel.begin() + first_[i], vel.begin() + first_[i + 1])});
        return out;
    }
    void integrate(double time, double step, void* hip_stream = nullptr) { check(rpt_particles_batch_integrate(h_, time, step, hip_stream)); }
    std::vector<std::vector<Vec3>> display_positions() const {
        std::vector<Vec3> all(first_.back());
        check(rpt_particles_batch_display_positions(h_, all[0].data()));
        std::vector<std::vector<Vec3>> out;
        for (size_t i = 0; i < size(); i++) out.emplace_back(all.begin() + first_[i], all.begin() + first_[i + 1]);
        return out;
    }
    // ... left in the ensemble's own device array (sum(n) x 3 doubles, the systems concatenated): asynchronous, ordered like integrate.
    void* display_positions_device(void* hip_stream = nullptr) const {
        void* d = nullptr;
        check(rpt_particles_batch_display_positions_device(h_, &d, hip_stream));
        return d;
    }
    std::vector<std::array<uint64_t, 8>> counters() const {
        std::vector<std::array<uint64_t, 8>> c(size());
        check(rpt_particles_batch_counters(h_, c[0].data()));
        return c;
    }
    std::array<uint64_t, 8> info() const {   // resident blocks, rounds, steps per launch, LDS bytes, largest n, particles, block, lanes
        std::array<uint64_t, 8> c{};
        check(rpt_particles_batch_info(h_, c.data()));
        return c;
    }
    rpt_particles_batch* raw() const { return h_; }

  private:
    rpt_particles_batch* h_ = nullptr;
    std::vector<size_t> first_;
};
// The three systems of particle_system.rs.  rk4_integrate goes through a handle on `device` (device < 0: the host function).
class BuiltinParticleSystem : public ParticleSystem {
  public:
    int device = 0;
    rpt_particles_params params(size_t n) const { return {kind_, uint32_t(n), radius_, height_}; }
    ParticleState time_derivative(const ParticleState& s) const override {
        ParticleState d{std::vector<Vec3>(s.size()), std::vector<Vec3>(s.size())};
        const rpt_particles_params prm = params(s.size());
        check(rpt_particles_derivative_host(&prm, s.size() ? s.pos[0].data() : nullptr, s.size() ? s.vel[0].data() : nullptr,
                                            s.size() ? d.pos[0].data() : nullptr, s.size() ? d.vel[0].data() : nullptr, nullptr));
        return d;
    }
    void rk4_integrate(ParticleState& s, double time, double step) const override {
        const rpt_particles_params prm = params(s.size());
        if (device < 0) {
            uint64_t c[8];
            check(rpt_particles_integrate_host(&prm, s.size() ? s.pos[0].data() : nullptr, s.size() ? s.vel[0].data() : nullptr, time, step, c));
            return;
        }
        ParticleSimulator sim(prm, s, device);
        sim.integrate(time, step);
        s = sim.state();
    }

  protected:
    BuiltinParticleSystem(int kind, double radius, double height) : kind_(kind), radius_(radius), height_(height) {}
    int32_t kind_;
    double radius_, height_;
};
struct SimpleCircleSystem : BuiltinParticleSystem {
    SimpleCircleSystem() : BuiltinParticleSystem(RPT_PARTICLES_CIRCLE, 0.0, 0.0) {}
};
struct SolidGravitySystem : BuiltinParticleSystem {
    SolidGravitySystem() : BuiltinParticleSystem(RPT_PARTICLES_GRAVITY, 0.0, 0.0) {}
};
struct MarblesSystem : BuiltinParticleSystem {
    explicit MarblesSystem(double radius, double height = 2.0) : BuiltinParticleSystem(RPT_PARTICLES_MARBLES, radius, height) {}
    std::vector<Vec3> display_positions(const std::vector<Vec3>& pos) const {   // marbles.rs:77-83 (a host function)
        std::vector<Vec3> out(pos.size());
        const rpt_particles_params prm = params(pos.size());
        check(rpt_particles_display_positions_host(&prm, pos.empty() ? nullptr : pos[0].data(), out.empty() ? nullptr : out[0].data()));
        return out;
    }
};

}  // namespace rpt

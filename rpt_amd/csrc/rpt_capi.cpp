// rpt_capi.cpp — host side of the C ABI (include/rpt_hip.h): fp64 scene store, flattening to
// the fp32 device layout (gpu_layout.h), BVH build for large meshes, launches.
#include <hip/hip_runtime_api.h>

#include <dlfcn.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <functional>
#include <limits>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "../../include/rpt_hip.h"
#include "scene_host.h"
#include "kernels.h"
#include "f64_layout.h"

using namespace rptg;

// ---------------------------------------------------------------------------- errors / options
static thread_local std::string g_err;
namespace rpti {
int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
}  // namespace rpti
using rpti::fail;
namespace rpti {
uint64_t seed_mix(uint64_t seed) {
    uint64_t x = seed + 0x9E3779B97F4A7C15ULL;
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ULL;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBULL;
    x ^= x >> 31;
    return x;
}
}  // namespace rpti
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e__ = (expr);                                                                   \
        if (e__ != hipSuccess)                                                                     \
            return fail(RPT_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e__));       \
    } while (0)

static rpt_options g_defaults;
static std::mutex g_defaults_mutex;
static int set_option_in(rpt_options& o, const char* name, int64_t value) {
    if (!name) return fail(RPT_ERR_INVALID, "null option name");
    const std::string s(name);
    if (s == "counters") o.counters = value;
    else if (s == "chunk_spp") { if (value < 0) return fail(RPT_ERR_INVALID, "chunk_spp must be >= 0 (0 = auto)"); o.chunk_spp = value; }
    else if (s == "blocks_per_cu") o.blocks_per_cu = value;
    else if (s == "max_blocks") { if (value < 0 || value > (1 << 20)) return fail(RPT_ERR_INVALID, "max_blocks must be 0..2^20 (0 = no cap)"); o.max_blocks = value; }
    else if (s == "timing") o.timing = value;
    else if (s == "room_shell") o.room_shell = value;
    else if (s == "scan_specialise") o.scan_specialise = value;
    else if (s == "scan_cull") o.scan_cull = value;
    else if (s == "shadow_scan") o.shadow_scan = value;
    else if (s == "scan_jit") { if (value < 0 || value > 2) return fail(RPT_ERR_INVALID, "scan_jit must be 0, 1 or 2"); o.scan_jit = value; }
    else if (s == "photon_skip") o.photon_skip = value;
    else if (s == "photon_block_lists") o.photon_block_lists = value;
    else if (s == "photon_parts") o.photon_parts = value;
    else if (s == "photon_keep_counts") { if (value < 0 || value > 1) return fail(RPT_ERR_INVALID, "photon_keep_counts must be 0 or 1"); o.photon_keep_counts = value; }
    else if (s == "photon_split") {
#ifndef RPT_EXPERIMENTS
        if (value != 0) return fail(RPT_ERR_UNSUPPORTED, "photon_split: a rejected prototype, built with -DRPT_EXPERIMENTS only");
#endif
        o.photon_split = value;
    }
    else if (s == "photon_coop_gather") o.photon_coop_gather = value;
    else if (s == "instancing") o.instancing = value;
    else if (s == "defer_lanes") { if (value < 1 || value > 64) return fail(RPT_ERR_INVALID, "defer_lanes must be 1..64"); o.defer_lanes = value; }
    else if (s == "bvh_leaf_max") { if (value < 1 || value > 16) return fail(RPT_ERR_INVALID, "bvh_leaf_max must be 1..16"); o.bvh_leaf_max = value; }
    else if (s == "bvh_sweep_below") { if (value < 0) return fail(RPT_ERR_INVALID, "bvh_sweep_below must be >= 0"); o.bvh_sweep_below = value; }
    else if (s == "bvh_max_depth") { if (value < 1 || value > 20) return fail(RPT_ERR_INVALID, "bvh_max_depth must be 1..20"); o.bvh_max_depth = value; }
    else if (s == "walk_leaf_quarters") { if (value < 0 || value > 256) return fail(RPT_ERR_INVALID, "walk_leaf_quarters must be 0..256"); o.walk_leaf_quarters = value; }
    else if (s == "detach_shadows") {
        if (value < 0 || value > 2) return fail(RPT_ERR_INVALID, "detach_shadows must be 0, 1 or 2");
#ifndef RPT_EXPERIMENTS
        if (value == 2) return fail(RPT_ERR_UNSUPPORTED, "detach_shadows = 2 (streamed walks): a rejected prototype, built with -DRPT_EXPERIMENTS only");
#endif
        o.detach_shadows = value;
    }
    else if (s == "stream_contexts") { if (value < 1 || value > 6) return fail(RPT_ERR_INVALID, "stream_contexts must be 1..6"); o.stream_contexts = value; }
    else if (s == "stream_backlog") { if (value < 1 || value > 256) return fail(RPT_ERR_INVALID, "stream_backlog must be 1..256"); o.stream_backlog = value; }
    else if (s == "detach_lanes") { if (value < 1 || value > 96) return fail(RPT_ERR_INVALID, "detach_lanes must be 1..96"); o.detach_lanes = value; }
    else if (s == "pull_batch") { if (value < 1 || value > 64) return fail(RPT_ERR_INVALID, "pull_batch must be 1..64"); o.pull_batch = value; }
    else if (s == "detach_trigger") { if (value < 1 || value > 32) return fail(RPT_ERR_INVALID, "detach_trigger must be 1..32"); o.detach_trigger = value; }
    else if (s == "defer_stop") { if (value < 1 || value > 64) return fail(RPT_ERR_INVALID, "defer_stop must be 1..64"); o.defer_stop = value; }
    else if (s == "f64_cull") { if (value < 0 || value > 2) return fail(RPT_ERR_INVALID, "f64_cull must be 0, 1 or 2"); o.f64_cull = value; }
    else if (s == "f64_mesh_tree_min") { if (value < 0 || value > (int64_t(1) << 32)) return fail(RPT_ERR_INVALID, "f64_mesh_tree_min must be 0..2^32"); o.f64_mesh_tree_min = value; }
    else if (s == "f64_photon_slice") { if (value < 0 || value > (1 << 20)) return fail(RPT_ERR_INVALID, "f64_photon_slice must be 0..2^20"); o.f64_photon_slice = value; }
    else if (s == "f64_surf_batch") { if (value < 1 || value > 64) return fail(RPT_ERR_INVALID, "f64_surf_batch must be 1..64"); o.f64_surf_batch = value; }
    else if (s == "epsilon_policy") { if (value < 0 || value > 1) return fail(RPT_ERR_INVALID, "epsilon_policy must be 0 or 1"); o.epsilon_policy = value; }
    else if (s == "denoise_stage") {
        if (value < -1 || value > int64_t(rptg::kDenoiseMaxStagedStep)) return fail(RPT_ERR_INVALID, "denoise_stage must be -1 (default), 0, 1 or 2");
        o.denoise_stage = value;
    }
    else if (s == "scene_tree_meshes") o.scene_tree_meshes = value;
    else if (s == "refit_per_height") { if (value < 0 || value > 1) return fail(RPT_ERR_INVALID, "refit_per_height must be 0 or 1"); o.refit_per_height = value; }
    else if (s == "scene_bvh_min") { if (value < 0) return fail(RPT_ERR_INVALID, "scene_bvh_min must be >= 0"); o.scene_bvh_min = value; }
    else return fail(RPT_ERR_INVALID, "unknown option: " + s);
    return RPT_OK;
}

// ---------------------------------------------------------------------------- fp64 helpers
namespace {
struct D3 {
    double x, y, z;
};
inline D3 operator+(D3 a, D3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline D3 operator-(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline D3 operator*(double s, D3 a) { return {s * a.x, s * a.y, s * a.z}; }
inline double dot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline D3 cross(D3 a, D3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline D3 normalize(D3 a) {
    double l = std::sqrt(dot(a, a));
    return {a.x / l, a.y / l, a.z / l};
}
inline D3 d3(const double* p) { return {p[0], p[1], p[2]}; }
// component by index.  (Not (&v.x)[a]: indexing past the member x is undefined, and clang does drop the
// y / z iterations of such a loop when it is not unrolled.)
inline double comp(const D3& v, int a) { return a == 0 ? v.x : (a == 1 ? v.y : v.z); }
inline F4 f4(D3 v, double w) { return F4{float(v.x), float(v.y), float(v.z), float(w)}; }
inline float bits_f(uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
inline uint32_t bits_u(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

// Derived matrices of Transformed::new (src/shape.rs:112-125), fp64.
struct Xf {
    bool has = false;
    double M[4][4], Minv[4][4], L[3][3], N[3][3], det = 1.0;
    D3 point(D3 p) const { return {M[0][0] * p.x + M[0][1] * p.y + M[0][2] * p.z + M[0][3], M[1][0] * p.x + M[1][1] * p.y + M[1][2] * p.z + M[1][3], M[2][0] * p.x + M[2][1] * p.y + M[2][2] * p.z + M[2][3]}; }
    D3 normal(D3 n) const { return {N[0][0] * n.x + N[0][1] * n.y + N[0][2] * n.z, N[1][0] * n.x + N[1][1] * n.y + N[1][2] * n.z, N[2][0] * n.x + N[2][1] * n.y + N[2][2] * n.z}; }
};
bool invert4(const double a[4][4], double out[4][4]) {
    double w[4][8];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            w[i][j] = a[i][j];
            w[i][4 + j] = i == j ? 1.0 : 0.0;
        }
    for (int c = 0; c < 4; c++) {
        int p = c;
        for (int r = c + 1; r < 4; r++)
            if (std::fabs(w[r][c]) > std::fabs(w[p][c])) p = r;
        if (w[p][c] == 0.0) return false;
        if (p != c)
            for (int j = 0; j < 8; j++) std::swap(w[p][j], w[c][j]);
        double d = w[c][c];
        for (int j = 0; j < 8; j++) w[c][j] /= d;
        for (int r = 0; r < 4; r++)
            if (r != c) {
                double f = w[r][c];
                if (f != 0.0)
                    for (int j = 0; j < 8; j++) w[r][j] -= f * w[c][j];
            }
    }
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) out[i][j] = w[i][4 + j];
    return true;
}
bool finish_xf(Xf& x);
bool make_xf(const rpt_shape_desc& d, Xf& x) {
    x.has = d.has_transform != 0;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) x.M[i][j] = x.has ? d.transform[i * 4 + j] : (i == j ? 1.0 : 0.0);
    return finish_xf(x);
}
// Transformed<KdTree<..Transformed<T>..>>: the child's matrix under the group's (world = P * C * local).
bool compose_xf(const Xf& parent, const rpt_shape_desc& d, Xf& x) {
    Xf c;
    if (!make_xf(d, c)) return false;
    x.has = parent.has || c.has;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            double a = 0.0;
            for (int k = 0; k < 4; k++) a += parent.M[i][k] * c.M[k][j];
            x.M[i][j] = (parent.has && c.has) ? a : (parent.has ? parent.M[i][j] : c.M[i][j]);
        }
    return finish_xf(x);
}
bool finish_xf(Xf& x) {
    if (!invert4(x.M, x.Minv)) return false;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) x.L[i][j] = x.M[i][j];
    const auto& a = x.L;
    x.det = a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) +
            a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]);
    if (x.det == 0.0 || !(x.det == x.det)) return false;
    // inverse transpose of the linear part
    double inv[3][3];
    inv[0][0] = (a[1][1] * a[2][2] - a[1][2] * a[2][1]) / x.det;
    inv[0][1] = (a[0][2] * a[2][1] - a[0][1] * a[2][2]) / x.det;
    inv[0][2] = (a[0][1] * a[1][2] - a[0][2] * a[1][1]) / x.det;
    inv[1][0] = (a[1][2] * a[2][0] - a[1][0] * a[2][2]) / x.det;
    inv[1][1] = (a[0][0] * a[2][2] - a[0][2] * a[2][0]) / x.det;
    inv[1][2] = (a[0][2] * a[1][0] - a[0][0] * a[1][2]) / x.det;
    inv[2][0] = (a[1][0] * a[2][1] - a[1][1] * a[2][0]) / x.det;
    inv[2][1] = (a[0][1] * a[2][0] - a[0][0] * a[2][1]) / x.det;
    inv[2][2] = (a[0][0] * a[1][1] - a[0][1] * a[1][0]) / x.det;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) x.N[i][j] = inv[j][i];
    return true;
}
D3 hex_color(uint32_t v) {  // src/color.rs:10-15
    auto ch = [](uint32_t c) { return std::pow(double(c) / 255.0, 2.2); };
    return {ch((v >> 16) & 0xff), ch((v >> 8) & 0xff), ch(v & 0xff)};
}
uint64_t mix64_(uint64_t x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ULL;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBULL;
    x ^= x >> 31;
    return x;
}
uint64_t seed_mix(uint64_t seed) { return rpti::seed_mix(seed); }

bool same_shape(const HShape& a, const HShape& b) {
    if (a.d.kind != b.d.kind || a.d.has_transform != b.d.has_transform) return false;
    if (a.d.has_transform && std::memcmp(a.d.transform, b.d.transform, sizeof(a.d.transform)) != 0) return false;
    if (a.d.kind == RPT_SHAPE_PLANE)
        return std::memcmp(a.d.plane_normal, b.d.plane_normal, 24) == 0 && a.d.plane_value == b.d.plane_value;
    if (a.d.kind == RPT_SHAPE_MONOMIAL) return std::memcmp(a.d.plane_normal, b.d.plane_normal, 16) == 0;   // height, exp
    if (a.d.kind == RPT_SHAPE_MESH)
        return a.mesh == b.mesh || (a.T().size() == b.T().size() &&
                                    (a.T().empty() || std::memcmp(a.T().data(), b.T().data(), a.T().size() * 8) == 0));
    if (a.d.kind == RPT_SHAPE_GROUP) {
        if (a.children.size() != b.children.size()) return false;
        for (size_t i = 0; i < a.children.size(); i++)
            if (!same_shape(a.children[i], b.children[i])) return false;
    }
    return true;
}

// ---------------------------------------------------------------------------- BVH build
struct BTri {
    float lo[3], hi[3], c[3];
    uint32_t idx;
};
struct TmpNode {  // build-time node: own box, children adjacent (left, left+1)
    float lo[3];
    uint32_t left_or_first;
    float hi[3];
    uint32_t count;  // 0 = inner
};
struct BvhBuilder {
    std::vector<BTri>& t;
    std::vector<TmpNode>& nodes;
    static constexpr int kBins = 16, kMaxDepth = 28;
    uint32_t leaf_max = 4;
    const std::vector<uint8_t>* solo = nullptr;  // by BTri::idx: items that must be alone in their leaf
    // The traversal keeps at most one stack entry per level and the stack has 32 (device_core.h): a tree that
    // comes out deeper than the caller can afford is rebuilt with `balanced` = object-median splits along the widest
    // centroid axis, whose depth is ceil(log2(n)) whatever the input looks like.
    bool balanced = false;
    int max_depth = 0;
    uint32_t sweep_below = 0;   // ranges of at most this many items: exact SAH sweep over the sorted centroids of each axis
    std::vector<float> sweep_area;
    // Exact SAH split of [first, first + count): the range is left sorted along the best axis, `mid` is the split.
    bool sweep_split(uint32_t first, uint32_t count, uint32_t& mid, float& cost_out) {
        float best = std::numeric_limits<float>::infinity();
        int best_axis = -1;
        uint32_t best_k = 0;
        sweep_area.resize(count);
        for (int a = 0; a < 3; a++) {
            std::sort(t.begin() + first, t.begin() + first + count, [a](const BTri& p, const BTri& q) { return p.c[a] < q.c[a] || (p.c[a] == q.c[a] && p.idx < q.idx); });
            float l0[3], h0[3];
            for (int k = 0; k < 3; k++) { l0[k] = std::numeric_limits<float>::infinity(); h0[k] = -l0[k]; }
            for (uint32_t i = count; i-- > 1;) {   // sweep_area[i] = area of items [i, count)
                for (int k = 0; k < 3; k++) { l0[k] = std::min(l0[k], t[first + i].lo[k]); h0[k] = std::max(h0[k], t[first + i].hi[k]); }
                sweep_area[i] = area(l0, h0);
            }
            for (int k = 0; k < 3; k++) { l0[k] = std::numeric_limits<float>::infinity(); h0[k] = -l0[k]; }
            for (uint32_t i = 1; i < count; i++) {   // left = [0, i), right = [i, count)
                for (int k = 0; k < 3; k++) { l0[k] = std::min(l0[k], t[first + i - 1].lo[k]); h0[k] = std::max(h0[k], t[first + i - 1].hi[k]); }
                const float cost = area(l0, h0) * float(i) + sweep_area[i] * float(count - i);
                if (cost < best) { best = cost; best_axis = a; best_k = i; }
            }
        }
        if (best_axis < 0) return false;
        if (best_axis != 2)
            std::sort(t.begin() + first, t.begin() + first + count, [best_axis](const BTri& p, const BTri& q) { return p.c[best_axis] < q.c[best_axis] || (p.c[best_axis] == q.c[best_axis] && p.idx < q.idx); });
        mid = first + best_k;
        cost_out = best;
        return true;
    }
    bool can_leaf(uint32_t first, uint32_t count) const {
        if (!solo || count == 1) return true;
        for (uint32_t i = first; i < first + count; i++)
            if ((*solo)[t[i].idx]) return false;
        return true;
    }
    void bounds(uint32_t first, uint32_t count, float lo[3], float hi[3], float clo[3], float chi[3]) {
        for (int a = 0; a < 3; a++) {
            lo[a] = clo[a] = std::numeric_limits<float>::infinity();
            hi[a] = chi[a] = -std::numeric_limits<float>::infinity();
        }
        for (uint32_t i = first; i < first + count; i++)
            for (int a = 0; a < 3; a++) {
                lo[a] = std::min(lo[a], t[i].lo[a]);
                hi[a] = std::max(hi[a], t[i].hi[a]);
                clo[a] = std::min(clo[a], t[i].c[a]);
                chi[a] = std::max(chi[a], t[i].c[a]);
            }
    }
    static float area(const float lo[3], const float hi[3]) {
        float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
        return dx * dy + dy * dz + dz * dx;
    }
    void build(uint32_t node, uint32_t first, uint32_t count, int depth) {
        float lo[3], hi[3], clo[3], chi[3];
        bounds(first, count, lo, hi, clo, chi);
        max_depth = std::max(max_depth, depth);
        TmpNode& n = nodes[node];
        for (int a = 0; a < 3; a++) {  // conservative padding for the fp32 slab test
            float pad = 1e-6f * std::max(std::fabs(lo[a]), std::fabs(hi[a])) + 1e-30f;
            n.lo[a] = lo[a] - pad;
            n.hi[a] = hi[a] + pad;
        }
        auto make_leaf = [&]() {
            nodes[node].left_or_first = first;
            nodes[node].count = count;
        };
        const bool leaf_ok = can_leaf(first, count);
        if (leaf_ok && (count <= leaf_max || (depth >= kMaxDepth && count <= 32))) return make_leaf();
        int best_axis = -1, best_bin = -1;
        float best_cost = std::numeric_limits<float>::infinity();
        uint32_t sweep_mid = 0;
        const bool swept = !balanced && count <= sweep_below && depth < kMaxDepth && sweep_split(first, count, sweep_mid, best_cost);
        for (int a = 0; a < 3 && !balanced && !swept; a++) {
            float ext = chi[a] - clo[a];
            if (!(ext > 0.f)) continue;
            uint32_t cnt[kBins] = {0};
            float blo[kBins][3], bhi[kBins][3];
            for (int b = 0; b < kBins; b++)
                for (int k = 0; k < 3; k++) {
                    blo[b][k] = std::numeric_limits<float>::infinity();
                    bhi[b][k] = -std::numeric_limits<float>::infinity();
                }
            float scale = float(kBins) / ext;
            for (uint32_t i = first; i < first + count; i++) {
                int b = std::min(kBins - 1, int((t[i].c[a] - clo[a]) * scale));
                cnt[b]++;
                for (int k = 0; k < 3; k++) {
                    blo[b][k] = std::min(blo[b][k], t[i].lo[k]);
                    bhi[b][k] = std::max(bhi[b][k], t[i].hi[k]);
                }
            }
            float la[kBins], ra[kBins];
            uint32_t lc[kBins], rc[kBins];
            float l0[3], h0[3];
            for (int k = 0; k < 3; k++) { l0[k] = std::numeric_limits<float>::infinity(); h0[k] = -l0[k]; }
            uint32_t c = 0;
            for (int b = 0; b < kBins; b++) {
                c += cnt[b];
                for (int k = 0; k < 3; k++) { l0[k] = std::min(l0[k], blo[b][k]); h0[k] = std::max(h0[k], bhi[b][k]); }
                lc[b] = c;
                la[b] = c ? area(l0, h0) : 0.f;
            }
            for (int k = 0; k < 3; k++) { l0[k] = std::numeric_limits<float>::infinity(); h0[k] = -l0[k]; }
            c = 0;
            for (int b = kBins - 1; b >= 0; b--) {
                c += cnt[b];
                for (int k = 0; k < 3; k++) { l0[k] = std::min(l0[k], blo[b][k]); h0[k] = std::max(h0[k], bhi[b][k]); }
                rc[b] = c;
                ra[b] = c ? area(l0, h0) : 0.f;
            }
            for (int b = 0; b < kBins - 1; b++) {
                if (lc[b] == 0 || rc[b + 1] == 0) continue;
                float cost = la[b] * float(lc[b]) + ra[b + 1] * float(rc[b + 1]);
                if (cost < best_cost) { best_cost = cost; best_axis = a; best_bin = b; }
            }
        }
        uint32_t mid;
        if (swept) {
            float parent_cost = area(lo, hi) * float(count);
            if (best_cost >= parent_cost && count <= 8 && leaf_ok) return make_leaf();
            mid = sweep_mid;
        } else if (balanced) {
            int axis = 0;
            for (int a = 1; a < 3; a++)
                if (chi[a] - clo[a] > chi[axis] - clo[axis]) axis = a;
            mid = first + count / 2;
            std::nth_element(t.begin() + first, t.begin() + mid, t.begin() + first + count,
                             [axis](const BTri& p, const BTri& q) { return p.c[axis] < q.c[axis]; });
        } else if (best_axis < 0 || depth >= kMaxDepth) {
            if (count <= 16 && leaf_ok) return make_leaf();
            mid = first + count / 2;  // all centroids coincide (or depth cap): split by index
        } else {
            float parent_cost = area(lo, hi) * float(count);
            if (best_cost >= parent_cost && count <= 8 && leaf_ok) return make_leaf();
            float ext = chi[best_axis] - clo[best_axis];
            float scale = float(kBins) / ext;
            auto it = std::partition(t.begin() + first, t.begin() + first + count, [&](const BTri& x) {
                int b = std::min(kBins - 1, int((x.c[best_axis] - clo[best_axis]) * scale));
                return b <= best_bin;
            });
            mid = uint32_t(it - t.begin());
            if (mid == first || mid == first + count) mid = first + count / 2;
        }
        uint32_t left = uint32_t(nodes.size());
        nodes.push_back(TmpNode{});
        nodes.push_back(TmpNode{});
        nodes[node].left_or_first = left;
        nodes[node].count = 0;
        build(left, first, mid - first, depth + 1);
        build(left + 1, mid, first + count - mid, depth + 1);
    }
};

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
};

}  // namespace


using MeshCallCache = std::unordered_map<const double*, std::pair<uint64_t, std::shared_ptr<const std::vector<double>>>>;
static std::shared_ptr<const std::vector<double>> intern_mesh(rpt_scene* s, const double* p, uint64_t n_tris,
                                                              MeshCallCache& seen) {
    auto it = seen.find(p);  // caller memory cannot change during one add call: same pointer, same data
    if (it != seen.end() && it->second.first == n_tris) return it->second.second;
    const size_t n = size_t(n_tris) * 18;
    uint64_t h = 0xCBF29CE484222325ULL ^ n;
    for (size_t i = 0; i < n; i++) {
        uint64_t w;
        std::memcpy(&w, p + i, 8);
        h = (h ^ w) * 0x100000001B3ULL;
        h ^= h >> 29;
    }
    auto& bucket = s->mesh_pool[h];
    for (auto& c : bucket)
        if (c->size() == n && std::memcmp(c->data(), p, n * 8) == 0) { seen[p] = {n_tris, c}; return c; }
    auto m = std::make_shared<const std::vector<double>>(p, p + n);
    bucket.push_back(m);
    seen[p] = {n_tris, m};
    return m;
}
static bool copy_shape(rpt_scene* s, MeshCallCache& seen, const rpt_shape_desc* d, HShape& out, std::string& why,
                       int depth = 0) {
    if (!d) { why = "null shape"; return false; }
    if (d->kind < 0 || d->kind > RPT_SHAPE_MONOMIAL) { why = "unknown shape kind"; return false; }
    if (d->kind == RPT_SHAPE_MONOMIAL && !std::isfinite(d->plane_normal[0])) { why = "MonomialSurface height must be finite"; return false; }
    out.d = *d;
    out.mesh.reset();
    out.children.clear();
    if (d->kind == RPT_SHAPE_MESH) {
        if (d->n_tris == 0 || !d->tris) { why = "mesh without triangles"; return false; }
        out.mesh = intern_mesh(s, d->tris, d->n_tris, seen);
    }
    if (d->kind == RPT_SHAPE_GROUP) {
        if (d->n_children == 0 || !d->children) { why = "group without children"; return false; }
        if (depth >= 16) { why = "groups nested too deeply"; return false; }
        out.children.resize(d->n_children);
        for (uint64_t i = 0; i < d->n_children; i++) {
            if (d->children[i].kind == RPT_SHAPE_PLANE) { why = "Plane is not Bounded and cannot be a KdTree child (src/kdtree.rs:12)"; return false; }
            if (!copy_shape(s, seen, d->children + i, out.children[i], why, depth + 1)) return false;
        }
    }
    out.d.tris = nullptr;
    out.d.children = nullptr;
    Xf x;
    if (!make_xf(*d, x)) { why = "singular transform"; return false; }
    return true;
}
static bool check_material(const rpt_material* m, std::string& why) {
    if (!m) { why = "null material"; return false; }
    if (m->kind < 0 || m->kind > RPT_MAT_TRANSMISSIVE) { why = "unknown material kind"; return false; }
    return true;
}

extern "C" {

const char* rpt_last_error(void) { return g_err.c_str(); }

int rpt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int rpt_set_option(const char* name, int64_t value) {
    std::lock_guard<std::mutex> lock(g_defaults_mutex);
    return set_option_in(g_defaults, name, value);
}
int rpt_scene_set_option(rpt_scene* s, const char* name, int64_t value) {
    if (!s) return fail(RPT_ERR_INVALID, "null scene");
    return set_option_in(s->opt, name, value);
}

rpt_scene* rpt_scene_create(void) {
    rpt_scene* s = new rpt_scene();
    std::lock_guard<std::mutex> lock(g_defaults_mutex);
    s->opt = g_defaults;
    return s;
}

// Everything a commit (and the renders after it) put on the device, freed on the scene's device; safe to repeat, and a
// commit that fails half-way (the reference-epsilon scene after the fp32 upload) leaves nothing behind.
static void release_device(rpt_scene* s) {
    if (!s->committed && !s->dev.arena && !s->dev.arena64) return;
    (void)hipSetDevice(s->device);
    s->dev = rpt_scene::Device{};
    if (s->photon) rpti::photon_release(s->photon);
    s->photon = nullptr;
    s->photon_stale = false;
    s->committed = false;
    s->jit = rpti::ScanJit{};   // (the modules belong to the process, not to the scene)
}

void rpt_scene_destroy(rpt_scene* s) {
    if (!s) return;
    release_device(s);
    delete s;
}

int rpt_scene_add_object(rpt_scene* s, const rpt_shape_desc* d, const rpt_material* m) {
    if (!s) return fail(RPT_ERR_INVALID, "null scene");
    if (s->committed) return fail(RPT_ERR_STATE, "scene is immutable after rpt_scene_commit");
    std::string why;
    HObject o;
    MeshCallCache seen;
    if (!copy_shape(s, seen, d, o.shape, why) || !check_material(m, why)) return fail(RPT_ERR_INVALID, why);
    o.mat = *m;
    s->objects.push_back(std::move(o));
    return int(s->objects.size()) - 1;
}
static int add_simple_light(rpt_scene* s, int kind, const double* color, const double* vec) {
    if (!s || !color) return fail(RPT_ERR_INVALID, "null argument");
    if (s->committed) return fail(RPT_ERR_STATE, "scene is immutable after rpt_scene_commit");
    HLight l{};
    l.kind = kind;
    std::memcpy(l.color, color, 24);
    if (vec) std::memcpy(l.vec, vec, 24);
    s->lights.push_back(std::move(l));
    return RPT_OK;
}
int rpt_scene_add_light_point(rpt_scene* s, const double color[3], const double location[3]) {
    if (!location) return fail(RPT_ERR_INVALID, "null location");
    return add_simple_light(s, L_POINT, color, location);
}
int rpt_scene_add_light_ambient(rpt_scene* s, const double color[3]) { return add_simple_light(s, L_AMBIENT, color, nullptr); }
int rpt_scene_add_light_directional(rpt_scene* s, const double color[3], const double direction[3]) {
    if (!direction) return fail(RPT_ERR_INVALID, "null direction");
    return add_simple_light(s, L_DIRECTIONAL, color, direction);
}
int rpt_scene_add_light_object(rpt_scene* s, const rpt_shape_desc* d, const rpt_material* m) {
    if (!s) return fail(RPT_ERR_INVALID, "null scene");
    if (s->committed) return fail(RPT_ERR_STATE, "scene is immutable after rpt_scene_commit");
    std::string why;
    HLight l{};
    l.kind = L_OBJECT;
    MeshCallCache seen;
    if (!copy_shape(s, seen, d, l.obj.shape, why) || !check_material(m, why)) return fail(RPT_ERR_INVALID, why);
    if (d->kind == RPT_SHAPE_PLANE)
        return fail(RPT_ERR_INVALID, "a plane cannot be a Light::Object (Plane::sample is unimplemented in rpt)");
    if (holds_monomial(l.obj.shape))
        return fail(RPT_ERR_UNSUPPORTED, "a MonomialSurface (alone or in a KdTree group) cannot be a Light::Object: MonomialSurface::sample "
                                         "is not built (src/shape/monomial_surface.rs:109-123)");
    l.obj.mat = *m;
    s->lights.push_back(std::move(l));
    return RPT_OK;
}
int rpt_scene_add_medium(rpt_scene* s, int32_t kind, double absorption, double scattering) {
    if (!s) return fail(RPT_ERR_INVALID, "null scene");
    if (s->committed) return fail(RPT_ERR_STATE, "scene is immutable after rpt_scene_commit");
    if (kind != RPT_MEDIUM_HOMOGENEOUS_ISOTROPIC && kind != RPT_MEDIUM_COLORED_GLOWING_FOG)
        return fail(RPT_ERR_INVALID, "unknown medium kind");
    if (!(absorption + scattering > 0.0)) return fail(RPT_ERR_INVALID, "medium extinction must be > 0");
    s->media.push_back(HMedium{kind, absorption, scattering});
    return RPT_OK;
}
int rpt_scene_set_environment_color(rpt_scene* s, const double rgb[3]) {
    if (!s || !rgb) return fail(RPT_ERR_INVALID, "null argument");
    if (s->committed) return fail(RPT_ERR_STATE, "scene is immutable after rpt_scene_commit");
    std::memcpy(s->env, rgb, 24);
    s->hdri_w = s->hdri_h = 0;
    s->hdri.clear();
    s->hdri64.clear();
    return RPT_OK;
}
int rpt_scene_set_environment_hdri(rpt_scene* s, uint32_t width, uint32_t height, const double* rgb) {
    if (!s || !rgb) return fail(RPT_ERR_INVALID, "null argument");
    if (s->committed) return fail(RPT_ERR_STATE, "scene is immutable after rpt_scene_commit");
    if (width == 0 || height == 0) return fail(RPT_ERR_INVALID, "Hdri::new asserts width > 0 && height > 0");
    s->hdri_w = width;
    s->hdri_h = height;
    s->hdri.resize(size_t(width) * height * 4);
    s->hdri64.assign(rgb, rgb + size_t(width) * height * 3);
    for (size_t i = 0; i < size_t(width) * height; i++) {
        s->hdri[4 * i] = float(rgb[3 * i]); s->hdri[4 * i + 1] = float(rgb[3 * i + 1]); s->hdri[4 * i + 2] = float(rgb[3 * i + 2]);
        s->hdri[4 * i + 3] = 0.f;
    }
    return RPT_OK;
}

// ---------------------------------------------------------------------------- commit (flatten + upload)
static const uint64_t kLinearTriMax = 32;  // meshes up to this size are scanned linearly (scalar loads)

static bool axis_aligned_positive(const Xf& x) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            if (i != j && x.M[i][j] != 0.0) return false;
    return x.M[0][0] > 0.0 && x.M[1][1] > 0.0 && x.M[2][2] > 0.0;
}

// Two consecutive flat, coplanar triangles of one mesh whose union is an axis-aligned rectangle
// (what polygon() produces for a wall): returns the axis (0/1/2) and fills the records, or -1.
static int detect_rect(const double* t0, const double* t1, const Xf& x, uint32_t obj, RectScan& rs, RectShade& rh) {
    for (int k = 1; k < 6; k++)  // all six vertex normals identical (flat, same plane orientation)
        if (std::memcmp(t0 + 9, (k < 3 ? t0 + 9 + 3 * k : t1 + 9 + 3 * (k - 3)), 24) != 0) return -1;
    D3 p[6] = {x.point(d3(t0)), x.point(d3(t0 + 3)), x.point(d3(t0 + 6)), x.point(d3(t1)), x.point(d3(t1 + 3)), x.point(d3(t1 + 6))};
    auto eq = [](const D3& a, const D3& b) { return a.x == b.x && a.y == b.y && a.z == b.z; };
    // the second triangle must share exactly two vertices with the first
    D3 q[4] = {p[0], p[1], p[2], p[0]};
    int shared = 0, extra = -1;
    for (int k = 3; k < 6; k++) {
        bool s = eq(p[k], p[0]) || eq(p[k], p[1]) || eq(p[k], p[2]);
        if (s) shared++;
        else extra = k;
    }
    if (shared != 2 || extra < 0) return -1;
    q[3] = p[extra];
    int lone = -1;  // vertex of the first triangle that is not on the shared edge
    for (int k = 0; k < 3; k++) {
        bool s = false;
        for (int m = 3; m < 6; m++) s = s || eq(p[k], p[m]);
        if (!s) lone = k;
    }
    if (lone < 0) return -1;
    for (int axis = 0; axis < 3; axis++) {
        auto c = [&](const D3& v, int a) { return comp(v, a % 3); };
        double pc = c(q[0], axis);
        if (c(q[1], axis) != pc || c(q[2], axis) != pc || c(q[3], axis) != pc) continue;
        int ua = axis + 1, va = axis + 2;
        double umin = c(q[0], ua), umax = umin, vmin = c(q[0], va), vmax = vmin;
        for (int k = 1; k < 4; k++) {
            umin = std::min(umin, c(q[k], ua)); umax = std::max(umax, c(q[k], ua));
            vmin = std::min(vmin, c(q[k], va)); vmax = std::max(vmax, c(q[k], va));
        }
        if (!(umax > umin && vmax > vmin)) return -1;
        int seen = 0;
        for (int k = 0; k < 4; k++) {
            double u = c(q[k], ua), v = c(q[k], va);
            if ((u != umin && u != umax) || (v != vmin && v != vmax)) return -1;
            seen |= 1 << ((u == umax ? 1 : 0) | (v == vmax ? 2 : 0));
        }
        if (seen != 15) return -1;
        // the unshared vertices must be opposite corners (so the shared edge is the other diagonal)
        const D3 &a = p[lone], &b = q[3];
        if (c(a, ua) == c(b, ua) || c(a, va) == c(b, va)) return -1;
        D3 n = x.has ? x.normal(d3(t0 + 9)) : d3(t0 + 9);
        n = normalize(n);
        rs.a = F4{float(pc), float(umin), float(umax), float(vmin)};
        rs.b = F4{float(vmax), 0.f, bits_f(obj), 0.f};
        rh.n_obj = f4(n, 0);
        rh.n_obj.w = bits_f(obj);
        return axis;
    }
    return -1;
}

static void push_tri(const double* t, const Xf& x, uint32_t obj, std::vector<TriScan>& scan,
                     std::vector<TriShade>& shade) {
    D3 v1 = x.point(d3(t)), v2 = x.point(d3(t + 3)), v3 = x.point(d3(t + 6));
    D3 n1 = d3(t + 9), n2 = d3(t + 12), n3 = d3(t + 15);
    bool flat = std::memcmp(t + 9, t + 12, 24) == 0 && std::memcmp(t + 9, t + 15, 24) == 0;
    D3 w1 = x.has ? x.normal(n1) : n1, w2 = x.has ? x.normal(n2) : n2, w3 = x.has ? x.normal(n3) : n3;
    D3 d0 = v2 - v1, d1 = v3 - v1;
    D3 pn = normalize(cross(d0, d1));
    double d00 = dot(d0, d0), d01 = dot(d0, d1), d11 = dot(d1, d1);
    double denom = d00 * d11 - d01 * d01;
    D3 A = (1.0 / denom) * (d11 * d0 - d01 * d1);
    D3 B = (1.0 / denom) * (d00 * d1 - d01 * d0);
    // tri_closer accepts u, v, w >= 0 of these functionals, evaluated in fp32 at an fp32 hit point: an error of about 1 ulp of the terms'
    // sum.  Two triangles that share an edge err independently there, and a ray within that error of the edge was rejected by both and
    // passed through the mesh.  So the functionals are those of the triangle enlarged about its centroid by e in every barycentric
    // coordinate ((v + e) / (1 + 3 e), likewise w and u), e = 4e-7 x the magnitude of the terms: neighbours overlap by the error.
    double aw = -dot(A, v1), bw = -dot(B, v1);
    const double big = std::max({std::fabs(v1.x), std::fabs(v1.y), std::fabs(v1.z), std::fabs(v2.x), std::fabs(v2.y), std::fabs(v2.z),
                                 std::fabs(v3.x), std::fabs(v3.y), std::fabs(v3.z)});
    const double sa = (std::fabs(A.x) + std::fabs(A.y) + std::fabs(A.z)) * big + std::fabs(aw) + 1.0;
    const double sb = (std::fabs(B.x) + std::fabs(B.y) + std::fabs(B.z)) * big + std::fabs(bw) + 1.0;
    const double e = 4e-7 * std::max(sa, sb), k = 1.0 / (1.0 + 3.0 * e);
    TriScan ts;
    ts.pn = f4(pn, dot(pn, v1));
    ts.A = f4(k * A, k * (aw + e));
    ts.B = f4(k * B, k * (bw + e));
    TriShade sh;
    if (flat) {
        sh.n1 = f4(normalize(w1), 0);
        sh.n2 = f4(D3{0, 0, 0}, 1.0);
        sh.n3 = f4(D3{0, 0, 0}, 0);
    } else {
        sh.n1 = f4(w1, 0);
        sh.n2 = f4(w2, 0.0);
        sh.n3 = f4(w3, 0);
    }
    sh.n1.w = bits_f(obj);
    scan.push_back(ts);
    shade.push_back(sh);
}

// ---------------------------------------------------------------------------- commit
// rpt_scene_commit = flatten_objects (records of every object + one tree per large mesh) -> flatten_lights ->
// fold_shell (flatten-time specialisation of the wall rectangles) -> mark_twin_ranges -> build_scene_tree ->
// collect_scan_boxes -> upload.  Everything before `upload` is pure host code over the fp64 scene;
// tests/host/flatten_harness.cpp runs the whole sequence with malloc-backed HIP stubs under ASan / UBSan.
namespace {
struct PBox { float lo[3], hi[3]; };   // world-space box of a bounded primitive
struct Flattener {
    rpt_scene* s;
    explicit Flattener(rpt_scene* scene) : s(scene) {}

    std::vector<XfScan> sph, cub;
    std::vector<XfShade> sph_sh, cub_sh;
    std::vector<PlaneScan> pln;
    std::vector<PlaneShade> pln_sh;
    std::vector<TriScan> tri, btri;
    std::vector<TriShade> tri_sh, btri_sh;
    std::vector<AabbScan> aabb;
    uint64_t sph_yrot = 0, cub_yrot = 0;   // specialise_scans
    std::vector<RectScan> rect_axis[3];
    std::vector<RectShade> rect_sh_axis[3];
    std::vector<BvhNode> nodes;
    std::vector<MeshRef> meshes;
    std::vector<Material> mats;
    std::vector<Light> lights;
    std::vector<LightTri> ltris;
    std::vector<LightXf> lxf;
    std::vector<LightPart> lparts;

    // world-space boxes of the bounded primitives (scene-level tree, scan boxes)
    std::vector<PBox> box_sph, box_cub, box_tri, box_mesh;
    std::vector<MonoScan> mono;       // monomial surfaces (scanned after the triangles)
    std::vector<XfShade> mono_sh;
    std::vector<PBox> box_mono;
    std::vector<InstRec> insts;
    std::vector<PBox> box_inst;
    std::unordered_map<const std::vector<double>*, uint32_t> mesh_uses;
    std::unordered_map<const std::vector<double>*, std::pair<MeshRef, PBox>> shared;
    int mesh_depth = 0, top_depth = 0;  // deepest mesh tree / the scene-level tree: their sum must fit the walk's stack
    // what the later stages leave
    ShellScan shell{};
    bool has_shell = false;
    std::vector<RectShade> shell_sh;   // shade records of the folded rectangles, in face order
    std::vector<RectScan> rect;        // the scanned rectangles, sorted by axis
    std::vector<RectShade> rect_sh;    // ... their shade records, followed by shell_sh
    std::vector<uint32_t> pleaf;
    // what a refit of the scene tree starts from (rpt_scene_set_movable_spheres): per entry of pleaf the box add_item received
    // (lo, hi), and per child entry of every scene-tree node (2 x local node + side) the bounds of the items below it, unpadded
    std::vector<float> pleaf_box, tree_raw;
    uint32_t top_root = 0;
    bool scene_bvh = false;
    bool mesh_deferred = false;   // the scene tree does not hold the meshes that have trees of their own
    std::vector<AabbScan> pbox;

    static PBox xf_box(const Xf& x, bool sphere) {  // unit sphere / unit cube under an affine map
        PBox b;
        for (int i = 0; i < 3; i++) {
            double h = 0.0;
            for (int j = 0; j < 3; j++) h += sphere ? x.M[i][j] * x.M[i][j] : 0.5 * std::fabs(x.M[i][j]);
            if (sphere) h = std::sqrt(h);
            h += 1e-5 * (h + std::fabs(x.M[i][3]));
            b.lo[i] = float(x.M[i][3] - h);
            b.hi[i] = float(x.M[i][3] + h);
        }
        return b;
    }
    static PBox mono_box(const Xf& x, double ylo, double yhi) {  // the local box [-1, ylo, -1]..[1, yhi, 1] under an affine map
        PBox b;
        for (int i = 0; i < 3; i++) {
            double lo = HUGE_VAL, hi = -HUGE_VAL;
            for (int c = 0; c < 8; c++) {
                const D3 q = x.point(D3{(c & 1) ? 1.0 : -1.0, (c & 2) ? yhi : ylo, (c & 4) ? 1.0 : -1.0});
                lo = std::min(lo, comp(q, i));
                hi = std::max(hi, comp(q, i));
            }
            const double pad = 1e-5 * (hi - lo + std::fabs(lo) + std::fabs(hi)) + 1e-30;
            b.lo[i] = std::nextafter(float(lo - pad), -std::numeric_limits<float>::infinity());
            b.hi[i] = std::nextafter(float(hi + pad), std::numeric_limits<float>::infinity());
        }
        return b;
    }
    static PBox tri_box(const double* t, const Xf& x) {
        PBox b;
        D3 v[3] = {x.point(d3(t)), x.point(d3(t + 3)), x.point(d3(t + 6))};
        for (int a = 0; a < 3; a++) {
            double c0 = comp(v[0], a), c1 = comp(v[1], a), c2 = comp(v[2], a);
            double lo = std::min(c0, std::min(c1, c2)), hi = std::max(c0, std::max(c1, c2));
            b.lo[a] = std::nextafter(float(lo), -std::numeric_limits<float>::infinity());
            b.hi[a] = std::nextafter(float(hi), std::numeric_limits<float>::infinity());
        }
        return b;
    }
    // Triangles of one mesh under `x` (identity for a shared mesh) + its two-box tree, appended to btri / nodes.
    MeshRef add_bvh_mesh(const std::vector<double>& mt, const Xf& x, uint32_t obj, PBox& box) {
        const uint64_t nt = mt.size() / 18;
        std::vector<TriScan> ms;
        std::vector<TriShade> mh;
        ms.reserve(nt);
        mh.reserve(nt);
        std::vector<BTri> bt(nt);
        for (uint64_t i = 0; i < nt; i++) {
            const double* t = &mt[i * 18];
            push_tri(t, x, obj, ms, mh);
            PBox tb = tri_box(t, x);
            for (int a = 0; a < 3; a++) {
                bt[i].lo[a] = tb.lo[a];
                bt[i].hi[a] = tb.hi[a];
                bt[i].c[a] = 0.5f * (tb.lo[a] + tb.hi[a]);
            }
            bt[i].idx = uint32_t(i);
        }
        MeshRef mr;
        mr.root = uint32_t(nodes.size());  // local node 0 is the root
        mr.tri_base = uint32_t(btri.size());
        mr.tri_count = uint32_t(nt);
        mr.object = obj;
        std::vector<TmpNode> tmp;
        tmp.reserve(nt);
        tmp.push_back(TmpNode{});
        int depth = 0;
        {
            BvhBuilder b{bt, tmp};
            b.leaf_max = uint32_t(s->opt.bvh_leaf_max);
            b.sweep_below = uint32_t(std::min<int64_t>(s->opt.bvh_sweep_below, 1 << 30));
            b.build(0, 0, uint32_t(nt), 0);
            depth = b.max_depth;
        }
        if (depth > s->opt.bvh_max_depth) {  // a chain-like SAH tree: the walk's stack could not hold it
            tmp.assign(1, TmpNode{});
            BvhBuilder b{bt, tmp};
            b.leaf_max = uint32_t(s->opt.bvh_leaf_max);
            b.sweep_below = 0;
            b.balanced = true;
            b.build(0, 0, uint32_t(nt), 0);
            depth = b.max_depth;
        }
        mesh_depth = std::max(mesh_depth, depth);
        // convert to two-box nodes: inner tmp node k -> wide node remap[k]
        std::vector<uint32_t> remap(tmp.size(), 0);
        uint32_t n_inner = 0;
        for (size_t k = 0; k < tmp.size(); k++)
            if (tmp[k].count == 0) remap[k] = n_inner++;
        std::vector<BvhNode> local(n_inner);
        auto entry = [&](uint32_t k) -> uint32_t {  // absolute node / triangle indices
            const TmpNode& c = tmp[k];
            if (c.count == 0) return mr.root + remap[k];
            return BVH_LEAF | ((c.count - 1u) << 26) | (mr.tri_base + c.left_or_first);
        };
        for (size_t k = 0; k < tmp.size(); k++) {
            if (tmp[k].count != 0) continue;
            BvhNode& w = local[remap[k]];
            uint32_t l = tmp[k].left_or_first;
            for (int a = 0; a < 3; a++) {
                w.lo0[a] = tmp[l].lo[a]; w.hi0[a] = tmp[l].hi[a];
                w.lo1[a] = tmp[l + 1].lo[a]; w.hi1[a] = tmp[l + 1].hi[a];
            }
            w.e0 = entry(l);
            w.e1 = entry(l + 1);
            w.pad0 = w.pad1 = 0;
        }
        for (uint64_t i = 0; i < nt; i++) {
            btri.push_back(ms[bt[i].idx]);
            btri_sh.push_back(mh[bt[i].idx]);
        }
        nodes.insert(nodes.end(), local.begin(), local.end());
        for (int a = 0; a < 3; a++) { box.lo[a] = tmp[0].lo[a]; box.hi[a] = tmp[0].hi[a]; }
        return mr;
    }
    void emit(const HShape& shape, const Xf& x, uint32_t obj) {
        switch (shape.d.kind) {
            case RPT_SHAPE_GROUP: {  // KdTree<Box<dyn Bounded>>: children become primitives of this object
                for (const HShape& c : shape.children) {
                    Xf cx;
                    compose_xf(x, c.d, cx);
                    emit(c, cx, obj);
                }
                break;
            }
            case RPT_SHAPE_SPHERE:
            case RPT_SHAPE_CUBE: {
                if (shape.d.kind == RPT_SHAPE_CUBE && axis_aligned_positive(x)) {
                    // positive scale + translation only: an axis-aligned box in world space
                    AabbScan b;
                    b.lo = F4{float(x.M[0][3] - 0.5 * x.M[0][0]), float(x.M[1][3] - 0.5 * x.M[1][1]),
                              float(x.M[2][3] - 0.5 * x.M[2][2]), bits_f(obj)};
                    b.hi = F4{float(x.M[0][3] + 0.5 * x.M[0][0]), float(x.M[1][3] + 0.5 * x.M[1][1]),
                              float(x.M[2][3] + 0.5 * x.M[2][2]), 0.f};
                    aabb.push_back(b);
                    break;
                }
                XfScan sc;
                sc.r0 = F4{float(x.Minv[0][0]), float(x.Minv[0][1]), float(x.Minv[0][2]), float(x.Minv[0][3])};
                sc.r1 = F4{float(x.Minv[1][0]), float(x.Minv[1][1]), float(x.Minv[1][2]), float(x.Minv[1][3])};
                sc.r2 = F4{float(x.Minv[2][0]), float(x.Minv[2][1]), float(x.Minv[2][2]), float(x.Minv[2][3])};
                XfShade sh;
                sh.r0 = F4{float(x.N[0][0]), float(x.N[0][1]), float(x.N[0][2]), bits_f(obj)};
                sh.r1 = F4{float(x.N[1][0]), float(x.N[1][1]), float(x.N[1][2]), x.has ? 1.f : 0.f};
                sh.r2 = F4{float(x.N[2][0]), float(x.N[2][1]), float(x.N[2][2]), 0.f};
                if (shape.d.kind == RPT_SHAPE_SPHERE) { sph.push_back(sc); sph_sh.push_back(sh); box_sph.push_back(xf_box(x, true)); }
                else { cub.push_back(sc); cub_sh.push_back(sh); box_cub.push_back(xf_box(x, false)); }
                break;
            }
            case RPT_SHAPE_MONOMIAL: {  // src/shape/monomial_surface.rs: local records, the box of :181-187 (min / max per axis)
                const double h = shape.d.plane_normal[0], ylo = std::min(0.0, h), yhi = std::max(0.0, h);
                MonoScan m;
                m.r0 = F4{float(x.Minv[0][0]), float(x.Minv[0][1]), float(x.Minv[0][2]), float(x.Minv[0][3])};
                m.r1 = F4{float(x.Minv[1][0]), float(x.Minv[1][1]), float(x.Minv[1][2]), float(x.Minv[1][3])};
                m.r2 = F4{float(x.Minv[2][0]), float(x.Minv[2][1]), float(x.Minv[2][2]), float(x.Minv[2][3])};
                m.h = F4{float(h), float(ylo), float(yhi), 0.f};
                XfShade sh;
                sh.r0 = F4{float(x.N[0][0]), float(x.N[0][1]), float(x.N[0][2]), bits_f(obj)};
                sh.r1 = F4{float(x.N[1][0]), float(x.N[1][1]), float(x.N[1][2]), x.has ? 1.f : 0.f};
                sh.r2 = F4{float(x.N[2][0]), float(x.N[2][1]), float(x.N[2][2]), 0.f};
                mono.push_back(m);
                mono_sh.push_back(sh);
                box_mono.push_back(mono_box(x, ylo, yhi));
                break;
            }
            case RPT_SHAPE_PLANE: {
                // world-space plane: (M^-T n) . x = value + (M^-T n) . translation
                D3 n = d3(shape.d.plane_normal);
                double value = shape.d.plane_value;
                if (x.has) {
                    D3 nw = x.normal(n);
                    value = value + dot(nw, D3{x.M[0][3], x.M[1][3], x.M[2][3]});
                    n = nw;
                }
                pln.push_back(PlaneScan{f4(n, value)});
                pln_sh.push_back(PlaneShade{f4(normalize(n), 0)});
                pln_sh.back().unit_n_obj.w = bits_f(obj);
                break;
            }
            default: {
                uint64_t nt = shape.T().size() / 18;
                if (nt <= kLinearTriMax) {
                    for (uint64_t i = 0; i < nt; i++) {
                        RectScan rs;
                        RectShade rh;
                        int axis = -1;
                        if (i + 1 < nt) axis = detect_rect(&shape.T()[i * 18], &shape.T()[(i + 1) * 18], x, obj, rs, rh);
                        if (axis >= 0) {
                            rect_axis[axis].push_back(rs);
                            rect_sh_axis[axis].push_back(rh);
                            i++;
                        } else {
                            push_tri(&shape.T()[i * 18], x, obj, tri, tri_sh);
                            box_tri.push_back(tri_box(&shape.T()[i * 18], x));
                        }
                    }
                } else if (s->opt.instancing && mesh_uses[shape.mesh.get()] >= 2) {
                    // shared mesh: one local-space tree, one InstRec per use
                    auto it = shared.find(shape.mesh.get());
                    if (it == shared.end()) {
                        Xf ident;
                        rpt_shape_desc none{};
                        make_xf(none, ident);
                        PBox lb;
                        MeshRef mr = add_bvh_mesh(shape.T(), ident, 0xFFFFFFFFu, lb);
                        it = shared.emplace(shape.mesh.get(), std::make_pair(mr, lb)).first;
                    }
                    const PBox& lb = it->second.second;
                    InstRec r;
                    r.r0 = F4{float(x.Minv[0][0]), float(x.Minv[0][1]), float(x.Minv[0][2]), float(x.Minv[0][3])};
                    r.r1 = F4{float(x.Minv[1][0]), float(x.Minv[1][1]), float(x.Minv[1][2]), float(x.Minv[1][3])};
                    r.r2 = F4{float(x.Minv[2][0]), float(x.Minv[2][1]), float(x.Minv[2][2]), float(x.Minv[2][3])};
                    r.n0 = F4{float(x.N[0][0]), float(x.N[0][1]), float(x.N[0][2]), bits_f(obj)};
                    r.n1 = F4{float(x.N[1][0]), float(x.N[1][1]), float(x.N[1][2]), bits_f(it->second.first.root)};
                    r.n2 = F4{float(x.N[2][0]), float(x.N[2][1]), float(x.N[2][2]), 0.f};
                    PBox wb;
                    for (int k = 0; k < 3; k++) { wb.lo[k] = std::numeric_limits<float>::infinity(); wb.hi[k] = -wb.lo[k]; }
                    for (int c = 0; c < 8; c++) {  // the instance's box: the local box's corners under the affine map
                        D3 q = x.point(D3{(c & 1) ? lb.hi[0] : lb.lo[0], (c & 2) ? lb.hi[1] : lb.lo[1], (c & 4) ? lb.hi[2] : lb.lo[2]});
                        const double qq[3] = {q.x, q.y, q.z};
                        for (int k = 0; k < 3; k++) {
                            double pad = 1e-5 * (std::fabs(qq[k]) + 1e-30);
                            wb.lo[k] = std::min(wb.lo[k], float(qq[k] - pad));
                            wb.hi[k] = std::max(wb.hi[k], float(qq[k] + pad));
                        }
                    }
                    insts.push_back(r);
                    box_inst.push_back(wb);
                } else {
                    PBox mb;
                    meshes.push_back(add_bvh_mesh(shape.T(), x, obj, mb));
                    box_mesh.push_back(mb);
                }
            }
        }
    }
    // (1) the records of every object, and one two-box tree per large mesh
    int flatten_objects() {
        // meshes referenced by more than one shape (Arc<Mesh> in the reference) are instanced
        std::function<void(const HShape&)> count_uses = [&](const HShape& shape) {
            if (shape.d.kind == RPT_SHAPE_MESH && shape.T().size() / 18 > kLinearTriMax) mesh_uses[shape.mesh.get()]++;
            for (const HShape& c : shape.children) count_uses(c);
        };
        for (const HObject& o : s->objects) count_uses(o.shape);
        for (size_t oi = 0; oi < s->objects.size(); oi++) {
            const HObject& o = s->objects[oi];
            Xf x;
            make_xf(o.shape.d, x);
            Material gm;
            gm.albedo_emit = F4{float(o.mat.albedo[0]), float(o.mat.albedo[1]), float(o.mat.albedo[2]), float(o.mat.emittance)};
            gm.params = F4{bits_f(uint32_t(o.mat.kind)), float(o.mat.shininess), float(o.mat.ior), 0.f};
            mats.push_back(gm);
            emit(o.shape, x, uint32_t(oi));
        }
        if (tri.size() >= BVH_INDEX_MASK || btri.size() >= BVH_INDEX_MASK || nodes.size() >= (1u << 30))
            return fail(RPT_ERR_UNSUPPORTED, "too many triangles");
        // the walk's stack column holds 21 entries in the per-mesh-tree kernels (a tree of depth d pushes at most d - 1)
        if (mesh_depth > 20) return fail(RPT_ERR_UNSUPPORTED, "a mesh tree is deeper than 20 levels even when rebuilt balanced (mesh too large)");

        return RPT_OK;
    }
    // (2) the light list in scene order (it fixes the RNG draw order) and the samplers' data
    void flatten_lights() {
        for (const HLight& hl : s->lights) {
            Light L{};
            L.kind = uint32_t(hl.kind);
            L.twin_object = -1;
            L.color = F4{float(hl.color[0]), float(hl.color[1]), float(hl.color[2]), 0.f};
            if (hl.kind == L_OBJECT) {
                const HObject& o = hl.obj;
                for (size_t j = 0; j < s->objects.size(); j++)
                    if (same_shape(o.shape, s->objects[j].shape)) { L.twin_object = int32_t(j); break; }
                // material.color() * material.emittance() (src/light.rs:41, material.rs:100-113)
                bool has = o.mat.kind == RPT_MAT_LAMBERTIAN || o.mat.kind == RPT_MAT_PHONG;
                double e = has ? o.mat.emittance : 0.0;
                L.color = F4{float(has ? o.mat.albedo[0] * e : 0.0), float(has ? o.mat.albedo[1] * e : 0.0),
                             float(has ? o.mat.albedo[2] * e : 0.0), 0.f};
                L.albedo = F4{float(has ? o.mat.albedo[0] : 0.0), float(has ? o.mat.albedo[1] : 0.0),
                              float(has ? o.mat.albedo[2] : 0.0), 0.f};
                // leaf shape -> LightXf (+ triangles); group -> parts tree (children contiguous, nested groups appended)
                std::function<LightPart(const HShape&, const Xf&)> light_part = [&](const HShape& shp, const Xf& x) -> LightPart {
                    LightPart part{};
                    if (shp.d.kind == RPT_SHAPE_GROUP) {
                        part.shape = LS_GROUP;
                        part.first = uint32_t(lparts.size());
                        part.count = uint32_t(shp.children.size());
                        lparts.resize(lparts.size() + shp.children.size());
                        for (size_t c = 0; c < shp.children.size(); c++) {
                            Xf cx;
                            compose_xf(x, shp.children[c].d, cx);
                            const LightPart child = light_part(shp.children[c], cx);  // may grow lparts: index, not reference
                            lparts[part.first + c] = child;
                        }
                        return part;
                    }
                    LightXf gx;
                    for (int r = 0; r < 3; r++) {
                        gx.fwd[r] = F4{float(x.M[r][0]), float(x.M[r][1]), float(x.M[r][2]), float(x.M[r][3])};
                        gx.inv[r] = F4{float(x.Minv[r][0]), float(x.Minv[r][1]), float(x.Minv[r][2]), float(x.Minv[r][3])};
                        gx.nrm[r] = F4{float(x.N[r][0]), float(x.N[r][1]), float(x.N[r][2]), 0.f};
                        gx.lin[r] = F4{float(x.L[r][0]), float(x.L[r][1]), float(x.L[r][2]), 0.f};
                    }
                    gx.nrm[0].w = float(x.det);
                    gx.nrm[1].w = x.has ? 1.f : 0.f;
                    part.xf = uint32_t(lxf.size());
                    lxf.push_back(gx);
                    if (shp.d.kind == RPT_SHAPE_MESH) {
                        part.shape = LS_MESH;
                        part.first = uint32_t(ltris.size());
                        const uint64_t nt = shp.T().size() / 18;
                        part.count = uint32_t(nt);
                        for (uint64_t i = 0; i < nt; i++) {
                            const double* t = &shp.T()[i * 18];
                            D3 a = d3(t), b = d3(t + 3), c = d3(t + 6);
                            D3 cr = cross(b - a, c - a);
                            double area = 0.5 * std::sqrt(dot(cr, cr));  // local-space area (src/shape/mesh.rs:93)
                            LightTri lt;
                            lt.v1 = f4(x.point(a), 1.0 / area);
                            lt.v2 = f4(x.point(b), 0);
                            lt.v3 = f4(x.point(c), 0);
                            lt.n1 = f4(d3(t + 9), 0);   // local normals; Transformed::sample maps them per sample
                            lt.n2 = f4(d3(t + 12), 0);
                            lt.n3 = f4(d3(t + 15), 0);
                            ltris.push_back(lt);
                        }
                    } else {
                        part.shape = shp.d.kind == RPT_SHAPE_SPHERE ? LS_SPHERE : LS_CUBE;
                    }
                    return part;
                };
                Xf x;
                make_xf(o.shape.d, x);
                const LightPart root = light_part(o.shape, x);
                L.shape = root.shape;
                L.first = root.first;
                L.count = root.count;
                L.xf = root.xf;
            }
            lights.push_back(L);
        }

    }
    // (3) flatten-time specialisation of the wall rectangles, then the final rectangle arrays
    void fold_shell() {
        // ---- box shell: rectangles that are exactly the faces of the box around all rectangles (the walls of a
        // room) leave the scanned list and are answered by one slab test; linear-scan scenes only
        const size_t n_items_total = sph.size() + cub.size() + aabb.size() + tri.size() + mono.size() + insts.size() + meshes.size() +
                                     rect_axis[0].size() + rect_axis[1].size() + rect_axis[2].size();
        const bool will_bvh = n_items_total >= size_t(std::max<int64_t>(2, s->opt.scene_bvh_min)) || !insts.empty();
        {
            const float inf = std::numeric_limits<float>::infinity();
            float blo[3] = {inf, inf, inf}, bhi[3] = {-inf, -inf, -inf};
            for (int a = 0; a < 3; a++)
                for (const RectScan& r : rect_axis[a]) {
                    const float lo[3] = {r.a.x, r.a.y, r.a.w}, hi[3] = {r.a.x, r.a.z, r.b.x};  // axis, u, v
                    for (int k = 0; k < 3; k++) {
                        blo[(a + k) % 3] = std::min(blo[(a + k) % 3], lo[k]);
                        bhi[(a + k) % 3] = std::max(bhi[(a + k) % 3], hi[k]);
                    }
                }
            int face_of[3][2] = {{-1, -1}, {-1, -1}, {-1, -1}}, n_faces = 0;  // index into rect_axis[a]
            if (!will_bvh && s->opt.room_shell)
                for (int a = 0; a < 3; a++)
                    for (size_t i = 0; i < rect_axis[a].size(); i++) {
                        const RectScan& r = rect_axis[a][i];
                        const int u = (a + 1) % 3, w = (a + 2) % 3;
                        if (r.a.y != blo[u] || r.a.z != bhi[u] || r.a.w != blo[w] || r.b.x != bhi[w]) continue;
                        for (int side = 0; side < 2; side++)
                            if (r.a.x == (side ? bhi[a] : blo[a]) && face_of[a][side] < 0 && blo[a] < bhi[a]) {
                                face_of[a][side] = int(i);
                                n_faces++;
                                break;
                            }
                    }
            if (n_faces >= 3) {
                has_shell = true;
                shell.lo = F4{blo[0], blo[1], blo[2], 0.f};
                shell.hi = F4{bhi[0], bhi[1], bhi[2], 0.f};
                for (int k = 0; k < 8; k++) shell.face[k] = CODE_MISS;
                size_t n_scanned = 0;
                for (int a = 0; a < 3; a++) n_scanned += rect_axis[a].size();
                n_scanned -= size_t(n_faces);
                for (int a = 0; a < 3; a++) {  // take the members out (higher index first, so indices stay valid)
                    int order[2] = {0, 1};
                    if (face_of[a][0] >= 0 && face_of[a][1] >= 0 && face_of[a][0] < face_of[a][1]) { order[0] = 1; order[1] = 0; }
                    RectShade keep[2];
                    for (int k = 0; k < 2; k++) {
                        const int side = order[k];
                        if (face_of[a][side] < 0) continue;
                        keep[side] = rect_sh_axis[a][size_t(face_of[a][side])];
                        rect_axis[a].erase(rect_axis[a].begin() + face_of[a][side]);
                        rect_sh_axis[a].erase(rect_sh_axis[a].begin() + face_of[a][side]);
                    }
                    for (int side = 0; side < 2; side++)
                        if (face_of[a][side] >= 0) {
                            shell.face[2 * a + side] = (K_RECT << 28) | uint32_t(n_scanned + shell_sh.size());
                            shell_sh.push_back(keep[side]);
                        }
                }
            }
        }
        // The scanned rectangles reach 2e-6 of their coordinates beyond their edges: rect_closer compares each rectangle's own fp32 hit point
        // with its own bounds, and where two walls meet in an edge of a room a ray at that edge overshot both (by up to 3 ulp of the
        // coordinate) and left the room.  (The shell's faces are gone from these lists: its slab test is closed.)
        for (int a = 0; a < 3; a++)
            for (RectScan& r : rect_axis[a]) {
                const float pu = 2e-6f * std::max(std::fabs(r.a.y), std::fabs(r.a.z)), pv = 2e-6f * std::max(std::fabs(r.a.w), std::fabs(r.b.x));
                r.a.y -= pu; r.a.z += pu; r.a.w -= pv; r.b.x += pv;
            }
        for (int a = 0; a < 3; a++) {
            rect.insert(rect.end(), rect_axis[a].begin(), rect_axis[a].end());
            rect_sh.insert(rect_sh.end(), rect_sh_axis[a].begin(), rect_sh_axis[a].end());
        }
        rect_sh.insert(rect_sh.end(), shell_sh.begin(), shell_sh.end());  // hit codes of shell faces point here
    }
    // (4) hit-code ranges of the lights' twin objects
    void mark_twin_ranges() {
        // ---- shadow test shortcut: when the primitives of a light's twin object form one contiguous range of
        // hit codes, "the closest hit belongs to the twin" is a range compare instead of a shade-record load
        for (Light& L : lights) {
            L.twin_lo = 1u;
            L.twin_hi = 0u;
            if (L.kind != L_OBJECT || L.twin_object < 0) continue;
            const uint32_t tw = uint32_t(L.twin_object);
            std::vector<uint32_t> codes;
            bool other = false;  // pieces a range cannot describe
            auto same = [&](float w) { return bits_u(w) == tw; };
            for (size_t i = 0; i < sph_sh.size(); i++) if (same(sph_sh[i].r0.w)) codes.push_back((K_SPHERE << 28) | uint32_t(i));
            for (size_t i = 0; i < cub_sh.size(); i++) if (same(cub_sh[i].r0.w)) codes.push_back((K_CUBE << 28) | uint32_t(i));
            for (size_t i = 0; i < pln_sh.size(); i++) if (same(pln_sh[i].unit_n_obj.w)) codes.push_back((K_PLANE << 28) | uint32_t(i));
            for (size_t i = 0; i < tri_sh.size(); i++) if (same(tri_sh[i].n1.w)) codes.push_back((K_TRI << 28) | uint32_t(i));
            for (size_t i = 0; i < aabb.size(); i++) if (same(aabb[i].lo.w)) codes.push_back((K_AABB << 28) | uint32_t(i));
            for (size_t i = 0; i < rect_sh.size(); i++) if (same(rect_sh[i].n_obj.w)) codes.push_back((K_RECT << 28) | uint32_t(i));
            for (const MeshRef& m : meshes) if (m.object == tw) other = true;
            for (const InstRec& r : insts) if (same(r.n0.w)) other = true;
            if (other || codes.empty()) continue;
            bool contiguous = true;
            for (size_t i = 1; i < codes.size(); i++) contiguous = contiguous && codes[i] == codes[i - 1] + 1u;
            if (contiguous) { L.twin_lo = codes.front(); L.twin_hi = codes.back(); }
        }
        // ---- the scans' shadow form (option "shadow_scan"; scan_prims<.., SHADOW>): for a light whose twin is one index range of ONE kind
        // that the linear scan tests record by record.  Not: a range that reaches the shell's faces (their codes follow the scanned
        // rectangles': the shell picks its face inside one test), planes (no light shape), anything in a tree, and no range at all (group
        // lights, monomial surfaces: they get no codes above).  Those lights keep the closest-hit scan.
        for (Light& L : lights) {
            L.color.w = 0.f;
            if (L.kind != L_OBJECT || L.twin_object < 0 || !(L.twin_lo <= L.twin_hi) || !s->opt.shadow_scan) continue;
            const uint32_t kind = L.twin_lo >> 28, last = L.twin_hi & 0x0FFFFFFFu;
            const bool one_kind = (L.twin_hi >> 28) == kind;
            const bool scanned = kind == K_SPHERE || kind == K_CUBE || kind == K_AABB || kind == K_TRI || (kind == K_RECT && last < rect.size());
            if (one_kind && scanned) L.color.w = bits_f(1u);
        }

    }
    // (5) the scene-level tree (many-primitive scenes only)
    int build_scene_tree() {
        // ---- scene-level BVH over bounded primitives and mesh roots (many-primitive scenes only)
        {
            std::vector<BTri> items;
            std::vector<uint32_t> codes;   // by item: primitive code, or K_BVHTRI << 28 | mesh index for a mesh root
            auto add_item = [&](const float lo[3], const float hi[3], uint32_t code) {
                BTri it;
                for (int a = 0; a < 3; a++) { it.lo[a] = lo[a]; it.hi[a] = hi[a]; it.c[a] = 0.5f * (lo[a] + hi[a]); }
                it.idx = uint32_t(codes.size());
                items.push_back(it);
                codes.push_back(code);
            };
            for (size_t i = 0; i < sph.size(); i++) add_item(box_sph[i].lo, box_sph[i].hi, (K_SPHERE << 28) | uint32_t(i));
            for (size_t i = 0; i < cub.size(); i++) add_item(box_cub[i].lo, box_cub[i].hi, (K_CUBE << 28) | uint32_t(i));
            for (size_t i = 0; i < aabb.size(); i++) {
                float lo[3] = {aabb[i].lo.x, aabb[i].lo.y, aabb[i].lo.z}, hi[3] = {aabb[i].hi.x, aabb[i].hi.y, aabb[i].hi.z};
                add_item(lo, hi, (K_AABB << 28) | uint32_t(i));
            }
            {
                size_t i = 0;
                for (int axis = 0; axis < 3; axis++)
                    for (size_t k = 0; k < rect_axis[axis].size(); k++, i++) {
                        const RectScan& r = rect[i];
                        float lo[3], hi[3];
                        lo[axis] = hi[axis] = r.a.x;
                        lo[(axis + 1) % 3] = r.a.y; hi[(axis + 1) % 3] = r.a.z;
                        lo[(axis + 2) % 3] = r.a.w; hi[(axis + 2) % 3] = r.b.x;
                        add_item(lo, hi, (K_RECT << 28) | uint32_t(i));
                    }
            }
            for (size_t i = 0; i < tri.size(); i++) add_item(box_tri[i].lo, box_tri[i].hi, (K_TRI << 28) | uint32_t(i));
            for (size_t i = 0; i < mono.size(); i++) add_item(box_mono[i].lo, box_mono[i].hi, (K_MONO << 28) | uint32_t(i));
            for (size_t i = 0; i < insts.size(); i++) add_item(box_inst[i].lo, box_inst[i].hi, (K_INST << 28) | uint32_t(i));
            std::vector<uint8_t> solo(items.size(), 0);
            // Meshes with trees of their own: leaves of the scene tree (option "scene_tree_meshes" = 1), or -- the default when
            // the tree has anything else to hold -- left outside it: a query then walks the scene tree for the small things and
            // the mesh trees separately, and the render kernel parks the mesh walks (kernels.hip, BVH = 3).
            const size_t n_counted = items.size() + meshes.size();   // (whether a tree is built does not depend on the option)
            mesh_deferred = !s->opt.scene_tree_meshes && !meshes.empty() && items.size() >= 2;
            if (!mesh_deferred)
                for (size_t i = 0; i < meshes.size(); i++) {
                    add_item(box_mesh[i].lo, box_mesh[i].hi, (K_BVHTRI << 28) | uint32_t(i));
                    solo.push_back(1);
                }
            if (n_counted >= size_t(std::max<int64_t>(2, s->opt.scene_bvh_min)) || !insts.empty()) {  // instances live in the tree only
                scene_bvh = true;
                std::vector<TmpNode> tmp;
                tmp.reserve(2 * items.size());
                // a mesh tree hangs below a leaf of this one (spliced in, or walked as an instance on the same stack)
                for (int attempt = 0; attempt < 2; attempt++) {
                    tmp.assign(1, TmpNode{});
                    BvhBuilder b{items, tmp};
                    b.leaf_max = 2;
                    b.solo = &solo;
                    b.balanced = attempt == 1;
                    b.build(0, 0, uint32_t(items.size()), 0);
                    top_depth = b.max_depth + 1;
                    if (top_depth + mesh_depth <= 31) break;
                }
                if (top_depth + mesh_depth > 31)
                    return fail(RPT_ERR_UNSUPPORTED, "scene tree + mesh tree are deeper than the traversal stack (32 levels)");
                std::vector<uint32_t> remap(tmp.size(), 0);
                uint32_t n_inner = 0;
                for (size_t k = 0; k < tmp.size(); k++)
                    if (tmp[k].count == 0) remap[k] = n_inner++;
                top_root = uint32_t(nodes.size());
                std::vector<BvhNode> local(n_inner);
                auto entry = [&](uint32_t k) -> uint32_t {
                    const TmpNode& c = tmp[k];
                    if (c.count == 0) return top_root + remap[k];
                    const uint32_t c0 = codes[items[c.left_or_first].idx];
                    if ((c0 >> 28) == K_BVHTRI) return meshes[c0 & 0x0FFFFFFFu].root;  // always alone in its leaf
                    const uint32_t first = uint32_t(pleaf.size());
                    for (uint32_t i = 0; i < c.count; i++) {
                        const BTri& it = items[c.left_or_first + i];
                        pleaf.push_back(codes[it.idx]);
                        pleaf_box.insert(pleaf_box.end(), it.lo, it.lo + 3);
                        pleaf_box.insert(pleaf_box.end(), it.hi, it.hi + 3);
                    }
                    return BVH_LEAF | BVH_PRIMS | ((c.count - 1u) << 26) | first;
                };
                // the bounds of the items below every tmp node before BvhBuilder::build pads them (children follow their parents)
                std::vector<PBox> raw(tmp.size());
                for (size_t k = tmp.size(); k-- > 0;) {
                    PBox& b = raw[k];
                    for (int a = 0; a < 3; a++) { b.lo[a] = std::numeric_limits<float>::infinity(); b.hi[a] = -b.lo[a]; }
                    const TmpNode& n = tmp[k];
                    for (uint32_t i = 0; i < (n.count == 0 ? 2u : n.count); i++) {
                        const float* lo = n.count == 0 ? raw[n.left_or_first + i].lo : items[n.left_or_first + i].lo;
                        const float* hi = n.count == 0 ? raw[n.left_or_first + i].hi : items[n.left_or_first + i].hi;
                        for (int a = 0; a < 3; a++) { b.lo[a] = std::min(b.lo[a], lo[a]); b.hi[a] = std::max(b.hi[a], hi[a]); }
                    }
                }
                tree_raw.assign(size_t(n_inner) * 12, 0.f);
                for (size_t k = 0; k < tmp.size(); k++) {
                    if (tmp[k].count != 0) continue;
                    BvhNode& w = local[remap[k]];
                    uint32_t l = tmp[k].left_or_first;
                    for (int a = 0; a < 3; a++) {
                        w.lo0[a] = tmp[l].lo[a]; w.hi0[a] = tmp[l].hi[a];
                        w.lo1[a] = tmp[l + 1].lo[a]; w.hi1[a] = tmp[l + 1].hi[a];
                    }
                    w.e0 = entry(l);
                    w.e1 = entry(l + 1);
                    w.pad0 = w.pad1 = 0;
                    for (uint32_t side = 0; side < 2; side++) {
                        float* r = &tree_raw[(size_t(remap[k]) * 2 + side) * 6];
                        for (int a = 0; a < 3; a++) { r[a] = raw[l + side].lo[a]; r[3 + a] = raw[l + side].hi[a]; }
                    }
                }
                nodes.insert(nodes.end(), local.begin(), local.end());
                if (pleaf.size() >= BVH_INDEX_MASK) return fail(RPT_ERR_UNSUPPORTED, "too many primitives");
            }
        }
        return RPT_OK;
    }
    // (5b) what the unmasked scans may leave out (SceneView::sph_yrot / cub_yrot, AabbScan::hi.w).  Nothing is reordered: record
    // order is the tie-break of the scans and defines the hit codes.  Only exact equalities of the fp32 values as stored count.
    static uint64_t yrot_mask(const std::vector<XfScan>& recs) {
        uint64_t m = 0;
        if (recs.size() > 64) return 0;   // (such a scene has a scene tree anyway)
        for (size_t i = 0; i < recs.size(); i++) {
            const XfScan& x = recs[i];
            if (x.r0.y == 0.f && x.r1.x == 0.f && x.r1.z == 0.f && x.r2.y == 0.f) m |= 1ull << i;
        }
        return m;
    }
    void specialise_scans() {
        sph_yrot = cub_yrot = 0;
        for (AabbScan& b : aabb) b.hi.w = 0.f;
        if (!s->opt.scan_specialise) return;
        sph_yrot = yrot_mask(sph);
        cub_yrot = yrot_mask(cub);
        for (size_t i = 0; i + 1 < aabb.size(); i += 2) {
            const AabbScan &a = aabb[i], &b = aabb[i + 1];
            uint32_t shared = 0;
            if (bits_u(a.lo.x) == bits_u(b.lo.x) && bits_u(a.hi.x) == bits_u(b.hi.x)) shared |= 1u;
            if (bits_u(a.lo.y) == bits_u(b.lo.y) && bits_u(a.hi.y) == bits_u(b.hi.y)) shared |= 2u;
            if (bits_u(a.lo.z) == bits_u(b.lo.z) && bits_u(a.hi.z) == bits_u(b.hi.z)) shared |= 4u;
            aabb[i].hi.w = bits_f(shared);
        }
    }
    // (6) boxes of the scanned records, for ball-limited queries
    void collect_scan_boxes() {
        // world boxes of the scanned bounded records, in scan order (SceneView::pbox)
        {
            auto push_box = [&](const float lo[3], const float hi[3]) {
                AabbScan b;
                float l[3], h[3];
                for (int a = 0; a < 3; a++) {
                    const float pad = 1e-5f * (std::fabs(lo[a]) + std::fabs(hi[a]) + (hi[a] - lo[a])) + 1e-7f;
                    l[a] = lo[a] - pad;
                    h[a] = hi[a] + pad;
                }
                b.lo = F4{l[0], l[1], l[2], 0.f};
                b.hi = F4{h[0], h[1], h[2], 0.f};
                pbox.push_back(b);
            };
            for (const PBox& b : box_sph) push_box(b.lo, b.hi);
            for (const PBox& b : box_cub) push_box(b.lo, b.hi);
            for (const AabbScan& b : aabb) { const float lo[3] = {b.lo.x, b.lo.y, b.lo.z}, hi[3] = {b.hi.x, b.hi.y, b.hi.z}; push_box(lo, hi); }
            size_t i = 0;
            for (int axis = 0; axis < 3; axis++)
                for (size_t k = 0; k < rect_axis[axis].size(); k++, i++) {   // the scanned rectangles (shell faces are gone)
                    const RectScan& r = rect[i];
                    float lo[3], hi[3];
                    lo[axis] = hi[axis] = r.a.x;
                    lo[(axis + 1) % 3] = r.a.y; hi[(axis + 1) % 3] = r.a.z;
                    lo[(axis + 2) % 3] = r.a.w; hi[(axis + 2) % 3] = r.b.x;
                    push_box(lo, hi);
                }
            for (const PBox& b : box_tri) push_box(b.lo, b.hi);
            for (const PBox& b : box_mono) push_box(b.lo, b.hi);   // (after the triangles; no masked scan reads them: device_core.h)
        }
    }
    // (6b) the box a culled primary scan tests before its tail (SceneView::scan_tail; option "scan_cull"), and, for the counters
    // build, the box around all scanned records and up to four candidate groups of records (scan_bound, scan_groups, scan_always:
    // what a finer cull would test -- measured, not built).  Nothing is reordered: a group is a box and a mask of record numbers in
    // the scan's numbering (= pbox order).
    //
    // Why a record that is left out could not have been hit.  A record is left out when the search interval [tmin, tbest) of every
    // lane misses a box B around the record's own box b.  Boxes (and the shell) are tested by the scan with t = (plane - o) * inv per
    // plane and fminf / fmaxf, the arithmetic of the box test itself: for planes P <= p, P - o <= p - o after rounding and the
    // product with the same inv keeps the order (fp32 rounding is monotone), a NaN (o in the plane, direction parallel to it) is
    // dropped by both alike, so the slab interval of b lies inside the one of B exactly and B needs no margin.  Every other kind
    // reaches its t through other operations: spheres and transformed cubes in local space, triangles through functionals solved
    // on the host, rectangles with a slab parameter on their own axis but a closed comparison of the hit point on the other two --
    // a ray that runs exactly in the plane of a rectangle's edge hits it, while the slab pair of a box that ends in that plane is
    // (NaN, +-inf) and misses.  Their relative errors are a few ulp of the coordinates involved, ~1e-6 of the scene's extent at
    // worst; their boxes are padded by 1e-4 of the extent, two orders of magnitude more, which also takes every such edge plane
    // off the faces of B.
    struct ScanGroupH { float lo[3], hi[3]; uint64_t mask; };
    std::vector<ScanGroupH> scan_groups;
    uint64_t scan_always = 0;
    float scan_lo[3] = {1, 0, 0}, scan_hi[3] = {0, 0, 0};   // lo > hi: no bound (the scene is not eligible)
    float tail_lo[3] = {0, 0, 0}, tail_hi[3] = {0, 0, 0};
    bool scan_cull = false;
    static double half_area(const float lo[3], const float hi[3]) {
        const double x = double(hi[0]) - lo[0], y = double(hi[1]) - lo[1], z = double(hi[2]) - lo[2];
        return x * y + y * z + z * x;
    }
    void group_scans() {
        scan_groups.clear();
        scan_always = 0;
        scan_cull = false;
        scan_lo[0] = 1.f; scan_hi[0] = 0.f;
        const size_t n_rect = rect.size();
        const size_t n = sph.size() + cub.size() + aabb.size() + n_rect + tri.size();
        if (scene_bvh || (n == 0 && !has_shell)) return;   // (a scene tree has taken the records)
        // the records' own boxes, in scan order; `local`: tested in local space or through solved functionals -> padded below
        std::vector<PBox> box;
        std::vector<bool> local;
        for (const PBox& b : box_sph) { box.push_back(b); local.push_back(true); }
        for (const PBox& b : box_cub) { box.push_back(b); local.push_back(true); }
        for (const AabbScan& b : aabb) { box.push_back(PBox{{b.lo.x, b.lo.y, b.lo.z}, {b.hi.x, b.hi.y, b.hi.z}}); local.push_back(false); }
        {
            size_t i = 0;
            for (int axis = 0; axis < 3; axis++)
                for (size_t k = 0; k < rect_axis[axis].size(); k++, i++) {
                    const RectScan& r = rect[i];
                    PBox b;
                    b.lo[axis] = b.hi[axis] = r.a.x;
                    b.lo[(axis + 1) % 3] = r.a.y; b.hi[(axis + 1) % 3] = r.a.z;
                    b.lo[(axis + 2) % 3] = r.a.w; b.hi[(axis + 2) % 3] = r.b.x;
                    box.push_back(b);
                    local.push_back(true);   // (its in-plane test is a comparison of the hit point, not a slab: see above)
                }
        }
        for (const PBox& b : box_tri) { box.push_back(b); local.push_back(true); }
        float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
        auto grow = [](float lo_[3], float hi_[3], const float blo[3], const float bhi[3]) {
            for (int a = 0; a < 3; a++) { lo_[a] = std::min(lo_[a], blo[a]); hi_[a] = std::max(hi_[a], bhi[a]); }
        };
        for (const PBox& b : box) grow(lo, hi, b.lo, b.hi);
        if (has_shell) { const float sl[3] = {shell.lo.x, shell.lo.y, shell.lo.z}, sh[3] = {shell.hi.x, shell.hi.y, shell.hi.z}; grow(lo, hi, sl, sh); }
        for (int a = 0; a < 3; a++)
            if (!(std::fabs(lo[a]) < FLT_MAX) || !(std::fabs(hi[a]) < FLT_MAX) || lo[a] > hi[a]) return;   // (a record without finite extent: no culling)
        const float pad = 1e-4f * std::max(hi[0] - lo[0], std::max(hi[1] - lo[1], hi[2] - lo[2]));
        for (size_t i = 0; i < box.size(); i++)
            if (local[i])
                for (int a = 0; a < 3; a++) { box[i].lo[a] -= pad; box[i].hi[a] += pad; }
        for (const PBox& b : box) grow(lo, hi, b.lo, b.hi);   // (the padded boxes as well)
        // the tail: what the scan tests after the shell
        const size_t n_tail = aabb.size() + n_rect + tri.size();
        if (n_tail != 0) {
            float tl[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, th[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
            for (size_t i = sph.size() + cub.size(); i < box.size(); i++) grow(tl, th, box[i].lo, box[i].hi);
            for (int a = 0; a < 3; a++) { tail_lo[a] = tl[a]; tail_hi[a] = th[a]; }
            scan_cull = s->opt.scan_cull != 0;
        }
        // the bound and the candidate groups of a finer cull, for the counters build (which classifies its trips by them whether
        // the option is on or off).  Planes are unbounded, monomial surfaces have no number, a mask has 64 bits.
        if (!pln.empty() || !mono.empty() || n > 64) return;
        for (int a = 0; a < 3; a++) { scan_lo[a] = lo[a]; scan_hi[a] = hi[a]; }
        // one group per record; a record whose box is most of the bound is always tested instead
        const double bound_area = half_area(lo, hi);
        for (size_t i = 0; i < box.size(); i++) {
            if (half_area(box[i].lo, box[i].hi) > 0.5 * bound_area) { scan_always |= 1ull << i; continue; }
            ScanGroupH g;
            for (int a = 0; a < 3; a++) { g.lo[a] = box[i].lo[a]; g.hi[a] = box[i].hi[a]; }
            g.mask = 1ull << i;
            scan_groups.push_back(g);
        }
        // merge the pair whose union has the smallest surface area (ties: the first pair in record order) until four are left
        while (scan_groups.size() > kMaxScanGroups) {
            size_t bi = 0, bj = 1;
            double best = -1.0;
            for (size_t i = 0; i < scan_groups.size(); i++)
                for (size_t j = i + 1; j < scan_groups.size(); j++) {
                    float ulo[3], uhi[3];
                    for (int a = 0; a < 3; a++) { ulo[a] = std::min(scan_groups[i].lo[a], scan_groups[j].lo[a]); uhi[a] = std::max(scan_groups[i].hi[a], scan_groups[j].hi[a]); }
                    const double ar = half_area(ulo, uhi);
                    if (best < 0.0 || ar < best) { best = ar; bi = i; bj = j; }
                }
            ScanGroupH& g = scan_groups[bi];
            const ScanGroupH& h = scan_groups[bj];
            for (int a = 0; a < 3; a++) { g.lo[a] = std::min(g.lo[a], h.lo[a]); g.hi[a] = std::max(g.hi[a], h.hi[a]); }
            g.mask |= h.mask;
            scan_groups.erase(scan_groups.begin() + long(bj));
        }
    }
    // (7) one arena for every array, the SceneView over it, statistics, per-launch scratch
    int upload(int device) {
        // ---- one arena for every array
        auto align = [](size_t v) { return (v + 255) & ~size_t(255); };
        size_t off = 0;
        auto reserve = [&](size_t bytes) {
            size_t o = off;
            off += align(std::max<size_t>(bytes, 16));
            return o;
        };
        size_t o_sph = reserve(sph.size() * sizeof(XfScan)), o_sphs = reserve(sph_sh.size() * sizeof(XfShade));
        size_t o_cub = reserve(cub.size() * sizeof(XfScan)), o_cubs = reserve(cub_sh.size() * sizeof(XfShade));
        size_t o_pln = reserve(pln.size() * sizeof(PlaneScan)), o_plns = reserve(pln_sh.size() * sizeof(PlaneShade));
        size_t o_tri = reserve(tri.size() * sizeof(TriScan)), o_tris = reserve(tri_sh.size() * sizeof(TriShade));
        size_t o_pbox = reserve(pbox.size() * sizeof(AabbScan));
        size_t o_pleaf = reserve(pleaf.size() * sizeof(uint32_t));
        size_t o_shell = reserve(sizeof(ShellScan));
        size_t o_inst = reserve(insts.size() * sizeof(InstRec));
        size_t o_aabb = reserve(aabb.size() * sizeof(AabbScan));
        size_t o_rect = reserve(rect.size() * sizeof(RectScan)), o_rects = reserve(rect_sh.size() * sizeof(RectShade));
        size_t o_nodes = reserve(nodes.size() * sizeof(BvhNode));
        size_t o_btri = reserve(btri.size() * sizeof(TriScan)), o_btris = reserve(btri_sh.size() * sizeof(TriShade));
        size_t o_mesh = reserve(meshes.size() * sizeof(MeshRef));
        size_t o_mats = reserve(mats.size() * sizeof(Material));
        size_t o_lights = reserve(lights.size() * sizeof(Light));
        size_t o_ltris = reserve(ltris.size() * sizeof(LightTri));
        size_t o_lxf = reserve(lxf.size() * sizeof(LightXf));
        size_t o_lparts = reserve(lparts.size() * sizeof(LightPart));
        size_t o_hdri = reserve(s->hdri.size() * sizeof(float));
        size_t o_mono = reserve(mono.size() * sizeof(MonoScan)), o_monos = reserve(mono_sh.size() * sizeof(XfShade));
        std::vector<char> host(off, 0);
        auto put = [&](size_t o, const void* src, size_t bytes) { if (bytes) std::memcpy(host.data() + o, src, bytes); };
        put(o_sph, sph.data(), sph.size() * sizeof(XfScan));       put(o_sphs, sph_sh.data(), sph_sh.size() * sizeof(XfShade));
        put(o_cub, cub.data(), cub.size() * sizeof(XfScan));       put(o_cubs, cub_sh.data(), cub_sh.size() * sizeof(XfShade));
        put(o_pln, pln.data(), pln.size() * sizeof(PlaneScan));    put(o_plns, pln_sh.data(), pln_sh.size() * sizeof(PlaneShade));
        put(o_tri, tri.data(), tri.size() * sizeof(TriScan));      put(o_tris, tri_sh.data(), tri_sh.size() * sizeof(TriShade));
        put(o_aabb, aabb.data(), aabb.size() * sizeof(AabbScan));
        put(o_pbox, pbox.data(), pbox.size() * sizeof(AabbScan));
        put(o_pleaf, pleaf.data(), pleaf.size() * sizeof(uint32_t));
        put(o_shell, &shell, sizeof(ShellScan));
        put(o_inst, insts.data(), insts.size() * sizeof(InstRec));
        put(o_rect, rect.data(), rect.size() * sizeof(RectScan));  put(o_rects, rect_sh.data(), rect_sh.size() * sizeof(RectShade));
        put(o_nodes, nodes.data(), nodes.size() * sizeof(BvhNode));
        put(o_btri, btri.data(), btri.size() * sizeof(TriScan));   put(o_btris, btri_sh.data(), btri_sh.size() * sizeof(TriShade));
        put(o_mesh, meshes.data(), meshes.size() * sizeof(MeshRef));
        put(o_mats, mats.data(), mats.size() * sizeof(Material));
        put(o_lights, lights.data(), lights.size() * sizeof(Light));
        put(o_ltris, ltris.data(), ltris.size() * sizeof(LightTri));
        put(o_lxf, lxf.data(), lxf.size() * sizeof(LightXf));
        put(o_lparts, lparts.data(), lparts.size() * sizeof(LightPart));
        put(o_hdri, s->hdri.data(), s->hdri.size() * sizeof(float));
        put(o_mono, mono.data(), mono.size() * sizeof(MonoScan));  put(o_monos, mono_sh.data(), mono_sh.size() * sizeof(XfShade));
        HIP_TRY(s->dev.arena.reserve(off));
        HIP_TRY(hipMemcpy(s->dev.arena.get(), host.data(), off, hipMemcpyHostToDevice));
        char* base = s->dev.arena.get<char>();
        SceneView& v = s->view;
        v.sph = (const XfScan*)(base + o_sph);      v.sph_sh = (const XfShade*)(base + o_sphs);    v.n_sph = uint32_t(sph.size());
        v.cub = (const XfScan*)(base + o_cub);      v.cub_sh = (const XfShade*)(base + o_cubs);    v.n_cub = uint32_t(cub.size());
        v.pln = (const PlaneScan*)(base + o_pln);   v.pln_sh = (const PlaneShade*)(base + o_plns); v.n_pln = uint32_t(pln.size());
        v.tri = (const TriScan*)(base + o_tri);     v.tri_sh = (const TriShade*)(base + o_tris);   v.n_tri = uint32_t(tri.size());
        v.aabb = (const AabbScan*)(base + o_aabb);  v.n_aabb = uint32_t(aabb.size());
        v.rect = (const RectScan*)(base + o_rect);  v.rect_sh = (const RectShade*)(base + o_rects);
        v.n_rect_x = uint32_t(rect_axis[0].size()); v.n_rect_y = uint32_t(rect_axis[1].size()); v.n_rect_z = uint32_t(rect_axis[2].size());
        v.shell = (const ShellScan*)(base + o_shell); v.has_shell = has_shell ? 1u : 0u;
        v.pbox = (const AabbScan*)(base + o_pbox);
        v.nodes = (const BvhNode*)(base + o_nodes); v.btri = (const TriScan*)(base + o_btri);      v.btri_sh = (const TriShade*)(base + o_btris);
        v.meshes = (const MeshRef*)(base + o_mesh); v.n_mesh = uint32_t(meshes.size());
        v.pleaf = (const uint32_t*)(base + o_pleaf); v.n_nodes = uint32_t(nodes.size());
        v.scene_bvh = scene_bvh ? 1u : 0u;          v.top_root = top_root;
        v.mesh_deferred = (scene_bvh && mesh_deferred) ? 1u : 0u;
        v.inst = (const InstRec*)(base + o_inst);   v.n_inst = uint32_t(insts.size());
        v.mono = (const MonoScan*)(base + o_mono);  v.mono_sh = (const XfShade*)(base + o_monos);  v.n_mono = uint32_t(mono.size());
        v.scan_pad_ = 0;  v.sph_yrot = sph_yrot;  v.cub_yrot = cub_yrot;
        v.scan_always = scan_always;
        std::memset(v.scan_groups, 0, sizeof(v.scan_groups));
        for (size_t g = 0; g < scan_groups.size(); g++) {
            for (int a = 0; a < 3; a++) { v.scan_groups[g].box.lo[a] = scan_groups[g].lo[a]; v.scan_groups[g].box.hi[a] = scan_groups[g].hi[a]; }
            v.scan_groups[g].mask = scan_groups[g].mask;
        }
        for (int a = 0; a < 3; a++) { v.scan_bound.lo[a] = scan_lo[a]; v.scan_bound.hi[a] = scan_hi[a]; v.scan_tail.lo[a] = tail_lo[a]; v.scan_tail.hi[a] = tail_hi[a]; }
        v.n_scan_groups = uint32_t(scan_groups.size());
        v.scan_cull = scan_cull ? 1u : 0u;
        v.scan_pad2_[0] = v.scan_pad2_[1] = 0;
        v.mats = (const Material*)(base + o_mats);  v.n_obj = uint32_t(mats.size());
        v.lights = (const Light*)(base + o_lights); v.n_lights = uint32_t(lights.size());
        v.ltris = (const LightTri*)(base + o_ltris); v.lxf = (const LightXf*)(base + o_lxf);
        v.lparts = (const LightPart*)(base + o_lparts); v.n_lparts = uint32_t(lparts.size());
        v.n_ltris = uint32_t(ltris.size());
        v.has_medium = s->media.empty() ? 0u : 1u;
        v.medium_kind = 0;
        v.sigma_a = v.sigma_s = 0.f;
        v.medium_emission = 0.f;
        v.medium_phase = 0.f;
        for (int i = 0; i < 3; i++) v.medium_color[i] = v.medium_color_hi[i] = 0.f;
        if (!s->media.empty()) {  // only media[0] is used (src/renderer.rs:190)
            const HMedium& m = s->media[0];
            v.medium_kind = uint32_t(m.kind);
            v.sigma_a = float(m.absorption);
            v.sigma_s = float(m.scattering);
            const double pi = 3.14159265358979323846;
            if (m.kind == RPT_MEDIUM_HOMOGENEOUS_ISOTROPIC) {  // src/medium.rs:80-96
                D3 c = hex_color(0xD2B48C);
                v.medium_color[0] = v.medium_color_hi[0] = float(c.x);
                v.medium_color[1] = v.medium_color_hi[1] = float(c.y);
                v.medium_color[2] = v.medium_color_hi[2] = float(c.z);
                v.medium_emission = 0.f;
                v.medium_phase = float(1.0 / (4.0 * pi));
            } else {  // colored_glowing_fog, src/medium.rs:99-122 (phase `1.0 / 4.0 * pi`, sic)
                D3 lo = hex_color(0x0000FF), hi = hex_color(0xFF0000);
                v.medium_color[0] = float(lo.x); v.medium_color[1] = float(lo.y); v.medium_color[2] = float(lo.z);
                v.medium_color_hi[0] = float(hi.x); v.medium_color_hi[1] = float(hi.y); v.medium_color_hi[2] = float(hi.z);
                v.medium_emission = 10.f;
                v.medium_phase = float(1.0 / 4.0 * pi);
            }
        }
        for (int i = 0; i < 3; i++) v.env[i] = float(s->env[i]);
        v.hdri = (const F4*)(base + o_hdri);
        v.hdri_w = s->hdri_w;
        v.hdri_h = s->hdri_h;
        s->prims_per_ray = sph.size() + cub.size() + pln.size() + tri.size() + aabb.size() + rect.size() + (has_shell ? 1 : 0);
        s->light_records = lights;
        s->jit.structure = rpti::scan_struct_of(rpti::scan_struct_default_groups(), lights, lxf, ltris.size(), mats, aabb, v.medium_kind, s->hdri_w != 0);
        s->twins_scanned = true;
        s->n_twin_lights = 0;
        for (const Light& L : lights) {
            if (L.kind == L_OBJECT && L.twin_object >= 0) s->n_twin_lights++;
            if (L.kind == L_OBJECT && L.twin_object >= 0 && !(L.twin_lo <= L.twin_hi)) s->twins_scanned = false;
        }
        s->stats[0] = sph.size(); s->stats[1] = cub.size(); s->stats[2] = pln.size(); s->stats[3] = tri.size();
        s->stats[4] = aabb.size(); s->stats[5] = rect_sh.size(); s->stats[6] = btri.size(); s->stats[7] = nodes.size();
        // scan-record bytes every closest-hit query walks (the uniform part of the algorithmic bytes)
        s->stats[8] = 48 * (sph.size() + cub.size() + tri.size()) + 16 * pln.size() + 32 * (aabb.size() + rect.size());
        s->stats[9] = off;
        s->stats[10] = scene_bvh ? (mesh_deferred ? 2 : 1) : 0;
        s->stats[11] = pleaf.size();
        s->stats[14] = has_shell ? shell_sh.size() : 0;
        s->stats[15] = uint64_t(top_depth + mesh_depth);
        s->stats[12] = insts.size();
        s->stats[13] = shared.size();

        for (auto& ls : s->dev.sets) {
            HIP_TRY(ls.d_queue.reserve(256));
            HIP_TRY(ls.done.create(hipEventDisableTiming));
            HIP_TRY(ls.launched.create(hipEventDisableTiming));
        }
        HIP_TRY(s->dev.d_counters.reserve(80 * sizeof(unsigned long long)));
        s->view.stack_overflows = s->dev.d_counters.get<unsigned long long>() + 7;
        s->pleaf_box = std::move(pleaf_box);
        s->tree_raw = std::move(tree_raw);
        s->device = device;
        s->committed = true;
        return RPT_OK;
    }
};
}  // namespace

// ---------------------------------------------------------------------------- reference-epsilon mode (f64_layout.h)
// The scene as the reference holds it: scene.objects in order, each a generic shape with the matrices Transformed::new
// derives (src/shape.rs:112-125), meshes as their triangles in local space, materials and lights in fp64.
// (What depends on a triangle alone is evaluated here with the reference's operations in the reference's order; the
// device must find the same bits, so nothing below may be contracted into an fma.)
#pragma clang fp contract(off)
static int check_scene64(const rpt_scene* s) {   // what the mode refuses, before anything is allocated
    std::function<int(const HShape&)> depth = [&](const HShape& h) {   // group levels around the deepest shape
        int d = 0;
        for (const HShape& c : h.children) d = std::max(d, depth(c));
        return d + (h.d.kind == RPT_SHAPE_GROUP ? 1 : 0);
    };
    for (const auto& o : s->objects)
        if (depth(o.shape) > int(rpt64::kMaxFrames))
            return fail(RPT_ERR_UNSUPPORTED, "epsilon_policy = 1 supports KdTree groups nested at most three deep");
    for (const auto& l : s->lights)
        if (l.kind == int(L_OBJECT) && depth(l.obj.shape) > int(rpt64::kMaxFrames))
            return fail(RPT_ERR_UNSUPPORTED, "epsilon_policy = 1 supports KdTree groups nested at most three deep");
    return RPT_OK;
}
static int fill_shape64(const HShape& hs, rpt64::Shape& o, std::vector<rpt64::Tri>& tris, std::vector<double>& tri_pdf,
                        std::unordered_map<const std::vector<double>*, uint32_t>* shared = nullptr) {
    std::memset(&o, 0, sizeof(o));
    o.kind = hs.d.kind;
    Xf x;
    if (!make_xf(hs.d, x)) return fail(RPT_ERR_INVALID, "singular transform");
    o.has_xf = x.has ? 1 : 0;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 4; j++) { o.inv[i * 4 + j] = x.Minv[i][j]; o.fwd[i * 4 + j] = x.M[i][j]; }
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) { o.lin[i * 3 + j] = x.L[i][j]; o.nrm[i * 3 + j] = x.N[i][j]; }
    o.det = x.det;
    for (int k = 0; k < 3; k++) o.plane[k] = hs.d.plane_normal[k];
    o.plane[3] = hs.d.plane_value;
    if (hs.d.kind == RPT_SHAPE_MESH) {
        const std::vector<double>& T = hs.T();
        // (an `Arc<Mesh>` used by several shapes keeps one copy of its triangles)
        const auto known = (shared && hs.mesh) ? shared->find(hs.mesh.get()) : decltype(shared->end()){};
        const bool have = shared && hs.mesh && known != shared->end();
        o.tri_first = have ? known->second : uint32_t(tris.size());
        o.tri_count = uint32_t(T.size() / 18);
        if (shared && hs.mesh && !have) (*shared)[hs.mesh.get()] = o.tri_first;
        for (int k = 0; k < 3; k++) { o.bmin[k] = std::numeric_limits<double>::infinity(); o.bmax[k] = -o.bmin[k]; }
        for (size_t t = 0; t < T.size() / 18; t++) {
            rpt64::Tri tr;
            std::memcpy(&tr, T.data() + t * 18, sizeof(tr));
            for (int v = 0; v < 3; v++)   // Triangle::bounding_box merged over the mesh (src/kdtree.rs:108-113)
                for (int k = 0; k < 3; k++) {
                    o.bmin[k] = std::min(o.bmin[k], T[t * 18 + v * 3 + k]);
                    o.bmax[k] = std::max(o.bmax[k], T[t * 18 + v * 3 + k]);
                }
            if (have) continue;
            tris.push_back(tr);
            // Triangle::sample's pdf (src/shape/mesh.rs:96-98) over KdTree::sample's choice (src/kdtree.rs:141-146)
            const double e0[3] = {tr.v2[0] - tr.v1[0], tr.v2[1] - tr.v1[1], tr.v2[2] - tr.v1[2]};
            const double e1[3] = {tr.v3[0] - tr.v1[0], tr.v3[1] - tr.v1[1], tr.v3[2] - tr.v1[2]};
            const double cx = e0[1] * e1[2] - e0[2] * e1[1], cy = e0[2] * e1[0] - e0[0] * e1[2], cz = e0[0] * e1[1] - e0[1] * e1[0];
            const double area = 0.5 * std::sqrt(cx * cx + cy * cy + cz * cz);
            tri_pdf.push_back((1.0 / area) / double(o.tri_count));
        }
    }
    return RPT_OK;
}
static void fill_mat64(const rpt_material& m, rpt64::Mat& o) {
    std::memset(&o, 0, sizeof(o));
    o.kind = m.kind;
    for (int k = 0; k < 3; k++) o.albedo[k] = m.albedo[k];
    o.emittance = m.emittance;
    o.shininess = m.shininess;
    o.ior = m.ior;
}
// What Triangle::intersect (src/shape/mesh.rs:50-83) computes from the triangle alone, by the same operations
static rpt64::TriRec tri_rec64(const rpt64::Tri& t) {
    rpt64::TriRec r;
    double d0[3], d1[3];
    for (int k = 0; k < 3; k++) { d0[k] = t.v2[k] - t.v1[k]; d1[k] = t.v3[k] - t.v1[k]; r.v1[k] = t.v1[k]; r.d0[k] = d0[k]; r.d1[k] = d1[k]; }
    const double c[3] = {d0[1] * d1[2] - d0[2] * d1[1], d0[2] * d1[0] - d0[0] * d1[2], d0[0] * d1[1] - d0[1] * d1[0]};
    const double len = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    for (int k = 0; k < 3; k++) r.pn[k] = c[k] / len;
    r.d00 = d0[0] * d0[0] + d0[1] * d0[1] + d0[2] * d0[2];
    r.d01 = d0[0] * d1[0] + d0[1] * d1[1] + d0[2] * d1[2];
    r.d11 = d1[0] * d1[0] + d1[1] * d1[1] + d1[2] * d1[2];
    r.denom = r.d00 * r.d11 - r.d01 * r.d01;
    return r;
}
// Padded world-space box of an object in fp32 (f64_layout.h, CullBox): the box of the shape's own bounds under its
// matrix, grown by 1e-5 of its size and of its coordinates, rounded outwards.
static rpt64::CullBox cull_box64(const rpt64::Shape& sh) {
    rpt64::CullBox c{};
    if (sh.kind == rpt64::SH_PLANE) { c.unbounded = 1u; return c; }
    double lo[3], hi[3];
    for (int k = 0; k < 3; k++) {
        const double h = sh.kind == rpt64::SH_SPHERE ? 1.0 : 0.5;
        lo[k] = sh.kind == rpt64::SH_MESH ? sh.bmin[k] : -h;
        hi[k] = sh.kind == rpt64::SH_MESH ? sh.bmax[k] : h;
        if (sh.kind == rpt64::SH_MONO) {   // src/shape/monomial_surface.rs:181-187, min / max per axis (a height <= 0 flips y)
            lo[k] = k == 1 ? std::min(0.0, sh.plane[0]) : -1.0;
            hi[k] = k == 1 ? std::max(0.0, sh.plane[0]) : 1.0;
        }
    }
    double wlo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, whi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    for (int corner = 0; corner < 8; corner++) {
        const double p[3] = {corner & 1 ? hi[0] : lo[0], corner & 2 ? hi[1] : lo[1], corner & 4 ? hi[2] : lo[2]};
        for (int i = 0; i < 3; i++) {
            const double w = sh.has_xf ? sh.fwd[i * 4] * p[0] + sh.fwd[i * 4 + 1] * p[1] + sh.fwd[i * 4 + 2] * p[2] + sh.fwd[i * 4 + 3] : p[i];
            wlo[i] = std::min(wlo[i], w);
            whi[i] = std::max(whi[i], w);
        }
    }
    double size = 0.0, mag = 0.0;
    for (int i = 0; i < 3; i++) { size = std::max(size, whi[i] - wlo[i]); mag = std::max(mag, std::max(std::fabs(wlo[i]), std::fabs(whi[i]))); }
    const double pad = 1e-5 * size + 1e-5 * mag + 1e-30;
    bool finite = true;
    for (int i = 0; i < 3; i++) {
        c.lo[i] = std::nextafter(float(wlo[i] - pad), -HUGE_VALF);
        c.hi[i] = std::nextafter(float(whi[i] + pad), HUGE_VALF);
        finite = finite && std::isfinite(c.lo[i]) && std::isfinite(c.hi[i]);
    }
    if (!finite) { c = rpt64::CullBox{}; c.unbounded = 1u; }   // (a box fp32 cannot hold: always evaluated)
    return c;
}
// Bounded::bounding_box of a shape in its parent's space (src/shape/*.rs, src/kdtree.rs:108-113, src/shape.rs:154-176: a
// Transformed shape's box is the box of the eight transformed corners of the inner box).
struct Box64 {
    double lo[3], hi[3];
};
static Box64 bbox64(const HShape& hs) {
    Box64 b;
    for (int k = 0; k < 3; k++) { b.lo[k] = std::numeric_limits<double>::infinity(); b.hi[k] = -b.lo[k]; }
    if (hs.d.kind == RPT_SHAPE_SPHERE || hs.d.kind == RPT_SHAPE_CUBE) {
        const double h = hs.d.kind == RPT_SHAPE_SPHERE ? 1.0 : 0.5;
        for (int k = 0; k < 3; k++) { b.lo[k] = -h; b.hi[k] = h; }
    } else if (hs.d.kind == RPT_SHAPE_MONOMIAL) {   // src/shape/monomial_surface.rs:181-187 (KdTree::new merges it with min / max)
        const double h = hs.d.plane_normal[0];
        for (int k = 0; k < 3; k++) { b.lo[k] = k == 1 ? std::min(0.0, h) : -1.0; b.hi[k] = k == 1 ? std::max(0.0, h) : 1.0; }
    } else if (hs.d.kind == RPT_SHAPE_MESH) {
        const std::vector<double>& T = hs.T();
        for (size_t t = 0; t < T.size() / 18; t++)
            for (int v = 0; v < 3; v++)
                for (int k = 0; k < 3; k++) {
                    b.lo[k] = std::min(b.lo[k], T[t * 18 + v * 3 + k]);
                    b.hi[k] = std::max(b.hi[k], T[t * 18 + v * 3 + k]);
                }
    } else if (hs.d.kind == RPT_SHAPE_GROUP) {
        for (const HShape& c : hs.children) {
            const Box64 cb = bbox64(c);
            for (int k = 0; k < 3; k++) { b.lo[k] = std::min(b.lo[k], cb.lo[k]); b.hi[k] = std::max(b.hi[k], cb.hi[k]); }
        }
    }
    if (!hs.d.has_transform) return b;
    Box64 w;
    for (int k = 0; k < 3; k++) { w.lo[k] = std::numeric_limits<double>::infinity(); w.hi[k] = -w.lo[k]; }
    const double* M = hs.d.transform;
    for (int c = 0; c < 8; c++) {
        const double p[3] = {c & 4 ? b.hi[0] : b.lo[0], c & 2 ? b.hi[1] : b.lo[1], c & 1 ? b.hi[2] : b.lo[2]};
        for (int i = 0; i < 3; i++) {
            const double v = M[i * 4] * p[0] + M[i * 4 + 1] * p[1] + M[i * 4 + 2] * p[2] + M[i * 4 + 3] * 1.0;
            w.lo[i] = std::min(w.lo[i], v);
            w.hi[i] = std::max(w.hi[i], v);
        }
    }
    return w;
}
struct Flat64 {
    std::unordered_map<const std::vector<double>*, uint32_t> shared_meshes;
    std::vector<rpt64::CullBox> cull;
    std::vector<rpt64::ObjRec> recs;
    std::vector<rpt64::ObjShade> shade;
    std::vector<rpt64::FrameRec> frames;
    std::vector<rpt64::FrameShade> fshade;
    std::vector<rpt64::Tri> tris;
    std::vector<double> tri_pdf;
};
// One shape of scene.objects[..] into records: a leaf becomes an ObjRec under the group levels in `chain`; a group adds a level and
// recurses.  `outer`: the forward matrices of the transformed levels above, outermost first (for the fp32 world box only).
static int flatten64(const HShape& hs, const rpt_material& mat, std::vector<uint32_t>& chain, std::vector<const double*>& outer, Flat64& F) {
    Xf x;
    if (!make_xf(hs.d, x)) return fail(RPT_ERR_INVALID, "singular transform");
    if (hs.d.kind == RPT_SHAPE_GROUP) {
        rpt64::FrameRec fr;
        rpt64::FrameShade fs;
        std::memset(&fr, 0, sizeof(fr));
        std::memset(&fs, 0, sizeof(fs));
        fs.has_xf = x.has ? 1 : 0;
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 4; j++) fr.inv[i * 4 + j] = x.Minv[i][j];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) fs.nrm[i * 3 + j] = x.N[i][j];
        HShape inner = hs;   // the group's bounds are those of KdTree::new: its children's boxes merged, in the group's own space
        inner.d.has_transform = 0;
        const Box64 gb = bbox64(inner);
        for (int k = 0; k < 3; k++) { fr.b[k] = gb.lo[k]; fr.b[3 + k] = gb.hi[k]; }
        chain.push_back(uint32_t(F.frames.size()));
        F.frames.push_back(fr);
        F.fshade.push_back(fs);
        if (x.has) outer.push_back(hs.d.transform);
        for (const HShape& c : hs.children)
            if (int rc = flatten64(c, mat, chain, outer, F)) return rc;
        if (x.has) outer.pop_back();
        chain.pop_back();
        return RPT_OK;
    }
    rpt64::Shape sh;
    if (int rc = fill_shape64(hs, sh, F.tris, F.tri_pdf, &F.shared_meshes)) return rc;
    rpt64::ObjRec r;
    std::memset(&r, 0, sizeof(r));
    r.kind = sh.kind; r.has_xf = sh.has_xf; r.tri_first = sh.tri_first; r.tri_count = sh.tri_count;
    r.n_frames = uint32_t(chain.size());
    for (size_t k = 0; k < chain.size(); k++) r.frame[k] = chain[k];
    for (int k = 0; k < 12; k++) r.inv[k] = sh.inv[k];
    for (int k = 0; k < 3; k++) {
        if (sh.kind == rpt64::SH_MESH) { r.b[k] = sh.bmin[k]; r.b[3 + k] = sh.bmax[k]; }
        else if (sh.kind == rpt64::SH_CUBE) { r.b[k] = -0.5; r.b[3 + k] = 0.5; }
        else if (sh.kind == rpt64::SH_PLANE) { r.b[k] = sh.plane[k]; }
        else if (sh.kind == rpt64::SH_MONO) { r.b[k] = k == 1 ? 0.0 : -1.0; r.b[3 + k] = k == 1 ? sh.plane[0] : 1.0; }   // p_min, p_max as given
    }
    if (sh.kind == rpt64::SH_PLANE) r.b[3] = sh.plane[3];
    // the fp32 world box: the shape's own box under its matrix, then under the groups' matrices, innermost first
    rpt64::CullBox cb = cull_box64(sh);
    cb.slab_test = sh.kind == rpt64::SH_CUBE ? 1u : 0u;
    if (!cb.unbounded && !outer.empty()) {
        double lo[3], hi[3];
        for (int k = 0; k < 3; k++) { lo[k] = cb.lo[k]; hi[k] = cb.hi[k]; }
        for (size_t lvl = outer.size(); lvl-- > 0;) {
            const double* M = outer[lvl];
            double wlo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, whi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
            for (int c = 0; c < 8; c++) {
                const double p[3] = {c & 1 ? hi[0] : lo[0], c & 2 ? hi[1] : lo[1], c & 4 ? hi[2] : lo[2]};
                for (int i = 0; i < 3; i++) {
                    const double v = M[i * 4] * p[0] + M[i * 4 + 1] * p[1] + M[i * 4 + 2] * p[2] + M[i * 4 + 3];
                    wlo[i] = std::min(wlo[i], v);
                    whi[i] = std::max(whi[i], v);
                }
            }
            for (int k = 0; k < 3; k++) { lo[k] = wlo[k]; hi[k] = whi[k]; }
        }
        double size = 0.0, mag = 0.0;
        for (int i = 0; i < 3; i++) { size = std::max(size, hi[i] - lo[i]); mag = std::max(mag, std::max(std::fabs(lo[i]), std::fabs(hi[i]))); }
        const double pad = 1e-5 * size + 1e-5 * mag + 1e-30;
        bool finite = true;
        for (int i = 0; i < 3; i++) {
            cb.lo[i] = std::nextafter(float(lo[i] - pad), -HUGE_VALF);
            cb.hi[i] = std::nextafter(float(hi[i] + pad), HUGE_VALF);
            finite = finite && std::isfinite(cb.lo[i]) && std::isfinite(cb.hi[i]);
        }
        if (!finite) { cb = rpt64::CullBox{}; cb.unbounded = 1u; }
    }
    rpt64::ObjShade os;
    std::memset(&os, 0, sizeof(os));
    for (int k = 0; k < 9; k++) os.nrm[k] = sh.nrm[k];
    fill_mat64(mat, os.mat);
    F.cull.push_back(cb);
    F.recs.push_back(r);
    F.shade.push_back(os);
    return RPT_OK;
}
// A light's shape tree (a KdTree group as Light::Object): `out` gets the group's record, its children a contiguous block of
// `pool` (their own children further back), so that KdTree::sample's choice is one index computation.
static int fill_light_shape64(const HShape& hs, rpt64::Shape& out, std::vector<rpt64::Shape>& pool, Flat64& F) {
    if (int rc = fill_shape64(hs, out, F.tris, F.tri_pdf, &F.shared_meshes)) return rc;
    if (hs.d.kind != RPT_SHAPE_GROUP) return RPT_OK;
    out.kind = rpt64::SH_GROUP;
    const size_t first = pool.size();
    out.tri_first = uint32_t(first);
    out.tri_count = uint32_t(hs.children.size());
    pool.resize(first + hs.children.size());
    for (size_t c = 0; c < hs.children.size(); c++) {
        rpt64::Shape child;   // (pool may grow while the child's own children are filled in)
        if (int rc = fill_light_shape64(hs.children[c], child, pool, F)) return rc;
        pool[first + c] = child;
    }
    return RPT_OK;
}
// The candidate trees of the reference-epsilon mode's meshes (f64_layout.h, MeshNode; kernels_f64.hip, mesh_tree_walk).
struct MeshTrees64 {
    std::vector<rpt64::MeshNode> nodes;
    std::vector<uint32_t> leaf;    // indices into trecs
    uint32_t n_meshes = 0, n_tris = 0;
    int depth = 0;
};
// One tree over triangles [first, first + count) of `tris` -- the mesh's own space, where Triangle::intersect runs --, appended to T;
// returns its root node + 1, 0 if the mesh is to keep the scan, or -1 (error set).  The topology is the fp32 path's builder's (on the
// triangles' boxes rounded to fp32; limited in depth the same way); the boxes are not: every node gets the fp64 box of its triangles'
// vertices, padded by CullBox's rule and rounded outwards, so a child's box lies inside its parent's and no box has a zero extent.
static int64_t build_mesh_tree64(const rpt_options& opt, const std::vector<rpt64::Tri>& tris, const std::vector<rpt64::TriRec>& trecs,
                                 uint32_t first, uint32_t count, MeshTrees64& T) {
    std::vector<BTri> bt(count);
    for (uint32_t i = 0; i < count; i++) {
        const rpt64::Tri& t = tris[first + i];
        const rpt64::TriRec& r = trecs[first + i];
        // a needle: the barycentric test of Triangle::intersect amplifies its rounding by d00 d11 / denom, and what it accepts need no longer
        // lie within the padding of the triangle's box.  (denom == 0 or NaN: v and w are inf / NaN and nothing is accepted.)
        if (r.denom != 0.0 && std::fabs(r.denom) < 1e-8 * r.d00 * r.d11) return 0;
        for (int a = 0; a < 3; a++) {
            const double lo = std::min(t.v1[a], std::min(t.v2[a], t.v3[a])), hi = std::max(t.v1[a], std::max(t.v2[a], t.v3[a]));
            if (!std::isfinite(float(lo)) || !std::isfinite(float(hi))) return 0;   // (NaN or beyond fp32: its CullBox is unbounded too)
            bt[i].lo[a] = float(lo);
            bt[i].hi[a] = float(hi);
            bt[i].c[a] = 0.5f * (bt[i].lo[a] + bt[i].hi[a]);
        }
        bt[i].idx = i;
    }
    const int max_depth = int(std::min<int64_t>(opt.bvh_max_depth, rpt64::kMeshTreeMaxDepth));
    std::vector<TmpNode> tmp;
    tmp.reserve(count);
    tmp.push_back(TmpNode{});
    int depth = 0;
    {
        BvhBuilder b{bt, tmp};
        b.leaf_max = uint32_t(opt.bvh_leaf_max);
        b.sweep_below = uint32_t(std::min<int64_t>(opt.bvh_sweep_below, 1 << 30));
        b.build(0, 0, count, 0);
        depth = b.max_depth;
    }
    if (depth > max_depth) {   // a chain-like SAH tree: the walk's stack could not hold it
        tmp.assign(1, TmpNode{});
        BvhBuilder b{bt, tmp};
        b.leaf_max = uint32_t(opt.bvh_leaf_max);
        b.balanced = true;
        b.build(0, 0, count, 0);
        depth = b.max_depth;
    }
    if (depth > max_depth) { fail(RPT_ERR_UNSUPPORTED, "mesh too large for the reference-epsilon mode's tree depth limit (raise bvh_leaf_max or bvh_max_depth)"); return -1; }
    const uint32_t node_base = uint32_t(T.nodes.size()), leaf_base = uint32_t(T.leaf.size());
    if (uint64_t(node_base) + tmp.size() >= (1ull << 31) || uint64_t(leaf_base) + count >= (1ull << 31)) { fail(RPT_ERR_UNSUPPORTED, "too many mesh tree nodes"); return -1; }
    T.nodes.resize(node_base + tmp.size());
    for (uint32_t i = 0; i < count; i++) T.leaf.push_back(first + bt[i].idx);
    std::vector<Box64> box(tmp.size());
    for (size_t k = tmp.size(); k-- > 0;) {   // children follow their parents in `tmp`: backwards, every child's box is known
        Box64& b = box[k];
        for (int a = 0; a < 3; a++) { b.lo[a] = std::numeric_limits<double>::infinity(); b.hi[a] = -b.lo[a]; }
        const TmpNode& n = tmp[k];
        if (n.count == 0) {
            for (uint32_t c = n.left_or_first; c < n.left_or_first + 2; c++)
                for (int a = 0; a < 3; a++) { b.lo[a] = std::min(b.lo[a], box[c].lo[a]); b.hi[a] = std::max(b.hi[a], box[c].hi[a]); }
        } else {
            for (uint32_t i = n.left_or_first; i < n.left_or_first + n.count; i++) {
                const rpt64::Tri& t = tris[first + bt[i].idx];
                for (const double* v : {t.v1, t.v2, t.v3})
                    for (int a = 0; a < 3; a++) { b.lo[a] = std::min(b.lo[a], v[a]); b.hi[a] = std::max(b.hi[a], v[a]); }
            }
        }
        double size = 0.0, mag = 0.0;
        for (int a = 0; a < 3; a++) { size = std::max(size, b.hi[a] - b.lo[a]); mag = std::max(mag, std::max(std::fabs(b.lo[a]), std::fabs(b.hi[a]))); }
        const double pad = 1e-5 * size + 1e-5 * mag + 1e-30;
        rpt64::MeshNode& o = T.nodes[node_base + k];
        for (int a = 0; a < 3; a++) {
            o.lo[a] = std::nextafter(float(b.lo[a] - pad), -HUGE_VALF);
            o.hi[a] = std::nextafter(float(b.hi[a] + pad), HUGE_VALF);
        }
        o.count = n.count;
        o.left_or_first = n.count == 0 ? node_base + n.left_or_first : leaf_base + n.left_or_first;
    }
    T.n_meshes++;
    T.n_tris += count;
    T.depth = std::max(T.depth, depth);
    return int64_t(node_base) + 1;
}
static int build_scene64(rpt_scene* s) {
    static_assert(sizeof(rpt64::Tri) == 18 * sizeof(double), "a triangle is its 18 doubles");
    if (int rc = check_scene64(s)) return rc;
    Flat64 F;
    for (size_t i = 0; i < s->objects.size(); i++) {
        std::vector<uint32_t> chain;
        std::vector<const double*> outer;
        if (int rc = flatten64(s->objects[i].shape, s->objects[i].mat, chain, outer, F)) return rc;
    }
    std::vector<rpt64::CullBox>& cull = F.cull;
    std::vector<rpt64::ObjRec>& recs = F.recs;
    std::vector<rpt64::ObjShade>& shade = F.shade;
    std::vector<rpt64::Tri>& tris = F.tris;
    std::vector<double>& tri_pdf = F.tri_pdf;
    const size_t n = recs.size();
    std::vector<rpt64::Light> lights(s->lights.size());
    std::vector<rpt64::Shape> lshapes;
    const size_t n_obj_tris = tris.size();
    std::vector<rpt64::TriRec> trecs(n_obj_tris);
    std::vector<rpt64::TriShade> tshade(n_obj_tris);
    for (size_t t = 0; t < n_obj_tris; t++) {
        trecs[t] = tri_rec64(tris[t]);
        for (int k = 0; k < 3; k++) { tshade[t].n1[k] = tris[t].n1[k]; tshade[t].n2[k] = tris[t].n2[k]; tshade[t].n3[k] = tris[t].n3[k]; }
    }
    for (size_t i = 0; i < s->lights.size(); i++) {
        const HLight& hl = s->lights[i];
        rpt64::Light& L = lights[i];
        std::memset(&L, 0, sizeof(L));
        L.kind = hl.kind;
        for (int k = 0; k < 3; k++) L.color[k] = hl.color[k];
        if (hl.kind == int(L_OBJECT)) {
            if (int rc = fill_light_shape64(hl.obj.shape, L.shape, lshapes, F)) return rc;
            fill_mat64(hl.obj.mat, L.mat);
        }
    }
    // the candidate trees: one per distinct mesh of at least f64_mesh_tree_min triangles (a mesh that shapes share is stored once)
    MeshTrees64 MT;
    std::vector<uint32_t> mroot;
    if (s->opt.f64_mesh_tree_min > 0 && s->opt.f64_cull != 0) {
        std::unordered_map<uint32_t, uint32_t> root_of;   // by tri_first
        for (size_t i = 0; i < n; i++) {
            const rpt64::ObjRec& r = recs[i];
            if (r.kind != rpt64::SH_MESH || int64_t(r.tri_count) < s->opt.f64_mesh_tree_min) continue;
            auto it = root_of.find(r.tri_first);
            if (it == root_of.end()) {
                const int64_t root = build_mesh_tree64(s->opt, tris, trecs, r.tri_first, r.tri_count, MT);
                if (root < 0) return int(RPT_ERR_UNSUPPORTED);
                it = root_of.emplace(r.tri_first, uint32_t(root)).first;
            }
            if (it->second != 0u) {
                if (mroot.empty()) mroot.assign(n, 0u);
                mroot[i] = it->second;
            }
        }
    }
    std::vector<rpt64::CullBox> cull_groups((n + 31) / 32);
    for (size_t g = 0; g < cull_groups.size(); g++) {
        rpt64::CullBox u{};
        for (int k = 0; k < 3; k++) { u.lo[k] = HUGE_VALF; u.hi[k] = -HUGE_VALF; }
        for (size_t i = 32 * g; i < std::min(n, 32 * g + 32); i++) {
            if (cull[i].unbounded) u.unbounded = 1u;
            if (cull[i].slab_test) u.slab_test = 2u;
            for (int k = 0; k < 3; k++) { u.lo[k] = std::min(u.lo[k], cull[i].lo[k]); u.hi[k] = std::max(u.hi[k], cull[i].hi[k]); }
        }
        if (u.unbounded) for (int k = 0; k < 3; k++) u.lo[k] = u.hi[k] = 0.f;
        cull_groups[g] = u;
    }
    struct Part { const void* src; size_t bytes, off; };
    Part parts[] = {{cull.data(), cull.size() * sizeof(rpt64::CullBox), 0},       {recs.data(), recs.size() * sizeof(rpt64::ObjRec), 0},
                    {shade.data(), shade.size() * sizeof(rpt64::ObjShade), 0},    {trecs.data(), trecs.size() * sizeof(rpt64::TriRec), 0},
                    {tshade.data(), tshade.size() * sizeof(rpt64::TriShade), 0},  {tris.data(), tris.size() * sizeof(rpt64::Tri), 0},
                    {tri_pdf.data(), tri_pdf.size() * sizeof(double), 0},         {lights.data(), lights.size() * sizeof(rpt64::Light), 0},
                    {F.frames.data(), F.frames.size() * sizeof(rpt64::FrameRec), 0}, {F.fshade.data(), F.fshade.size() * sizeof(rpt64::FrameShade), 0},
                    {s->hdri64.data(), s->hdri64.size() * sizeof(double), 0},
                    {cull_groups.data(), cull_groups.size() * sizeof(rpt64::CullBox), 0},
                    {lshapes.data(), lshapes.size() * sizeof(rpt64::Shape), 0},
                    {MT.nodes.data(), MT.nodes.size() * sizeof(rpt64::MeshNode), 0},
                    {MT.leaf.data(), MT.leaf.size() * sizeof(uint32_t), 0},
                    {mroot.data(), mroot.size() * sizeof(uint32_t), 0}};
    size_t total = 0;
    for (auto& p : parts) { p.off = total; total = (total + p.bytes + 255) & ~size_t(255); }
    total = std::max<size_t>(total, 256);
    HIP_TRY(s->dev.arena64.reserve(total));
    HIP_TRY(hipMemset(s->dev.arena64.get(), 0, total));   // (the gaps between the arrays too: the host tests checksum the arena)
    char* base = s->dev.arena64.get<char>();
    for (auto& p : parts)
        if (p.bytes) HIP_TRY(hipMemcpy(base + p.off, p.src, p.bytes, hipMemcpyHostToDevice));
    rpt64::Scene& v = s->view64;
    v.cull = reinterpret_cast<const rpt64::CullBox*>(base + parts[0].off);
    v.recs = reinterpret_cast<const rpt64::ObjRec*>(base + parts[1].off);
    v.shade = reinterpret_cast<const rpt64::ObjShade*>(base + parts[2].off);
    v.trecs = reinterpret_cast<const rpt64::TriRec*>(base + parts[3].off);
    v.tshade = reinterpret_cast<const rpt64::TriShade*>(base + parts[4].off);
    v.tris = reinterpret_cast<const rpt64::Tri*>(base + parts[5].off);
    v.tri_pdf = reinterpret_cast<const double*>(base + parts[6].off);
    v.lights = reinterpret_cast<const rpt64::Light*>(base + parts[7].off);
    v.frames = reinterpret_cast<const rpt64::FrameRec*>(base + parts[8].off);
    v.fshade = reinterpret_cast<const rpt64::FrameShade*>(base + parts[9].off);
    v.hdri = reinterpret_cast<const double*>(base + parts[10].off);
    v.cull32 = reinterpret_cast<const rpt64::CullBox*>(base + parts[11].off);
    v.lshapes = reinterpret_cast<const rpt64::Shape*>(base + parts[12].off);
    s->mnodes64 = reinterpret_cast<const rpt64::MeshNode*>(base + parts[13].off);
    s->mleaf64 = reinterpret_cast<const uint32_t*>(base + parts[14].off);
    s->mroot64 = mroot.empty() ? nullptr : reinterpret_cast<const uint32_t*>(base + parts[15].off);
    {
        // which passes walk the trees: the render and intersect kernels, unless the scene needs the group-light or the monomial flavour
        // (those, and the photon passes of the mode, scan every triangle as before)
        bool other_flavour = false;
        for (const auto& l : s->lights)
            if (l.kind == int(L_OBJECT) && l.obj.shape.d.kind == RPT_SHAPE_GROUP) other_flavour = true;
        for (const auto& o : s->objects)
            if (holds_monomial(o.shape)) other_flavour = true;
        uint64_t* I = s->mesh_tree_info64;
        I[0] = MT.n_meshes; I[1] = MT.n_tris; I[2] = MT.nodes.size(); I[3] = uint64_t(MT.depth);
        I[4] = parts[13].bytes + parts[14].bytes + parts[15].bytes;
        I[5] = (MT.n_meshes != 0 && !other_flavour) ? 1 : 0;
        I[6] = 0;
        I[7] = uint64_t(s->opt.f64_mesh_tree_min);
    }
    v.hdri_w = s->hdri64.empty() ? 0u : s->hdri_w;
    v.hdri_h = s->hdri64.empty() ? 0u : s->hdri_h;
    v.n_objects = uint32_t(n);
    // the buckets of the cubes' face coordinates (f64_layout.h, Scene::face_bits; the tolerance is cull32's, kernels_f64.hip)
    for (int k = 0; k < 3; k++) {
        float lo = HUGE_VALF, hi = -HUGE_VALF;
        for (size_t i = 0; i < n; i++)
            if (cull[i].slab_test && !cull[i].unbounded) { lo = std::min(lo, cull[i].lo[k]); hi = std::max(hi, cull[i].hi[k]); }
        v.face_bits[k] = 0;
        v.face_base[k] = 0.f;
        v.face_inv_cell[k] = 0.f;
        if (!(lo <= hi)) continue;   // no cube: no bucket is marked
        float tol_max = 0.f;
        for (size_t i = 0; i < n; i++)
            if (cull[i].slab_test && !cull[i].unbounded) {
                float size = 0.f, mag = 0.f;
                for (int a = 0; a < 3; a++) { size = std::max(size, cull[i].hi[a] - cull[i].lo[a]); mag = std::max({mag, std::fabs(cull[i].lo[a]), std::fabs(cull[i].hi[a])}); }
                tol_max = std::max(tol_max, 5e-5f * (size + mag));
            }
        const float mag_all = std::max(std::fabs(lo), std::fabs(hi));
        const float T = 2.f * tol_max + 4e-6f * mag_all + 1e-30f;   // cull32's tolerance (its `eo` is 1e-6 of the origin, which lies within T of the face), twice
        const float base = lo - 2.f * T, span = (hi + 2.f * T) - base;
        const float inv = 64.f / (span * 1.0001f);
        v.face_base[k] = base;
        v.face_inv_cell[k] = inv;
        auto mark = [&](float c) {
            for (float x : {c - T, c, c + T}) {
                const float f = (x - base) * inv;
                if (f >= 0.f && f < 64.f) v.face_bits[k] |= 1ull << unsigned(f);
            }
            // (c - T and c + T may lie more than one bucket apart when the buckets are narrower than 2 T: mark the run)
            const float f0 = std::max((c - T - base) * inv, 0.f), f1 = std::min((c + T - base) * inv, 63.f);
            for (int b = int(f0); b <= int(f1); b++) v.face_bits[k] |= 1ull << unsigned(b);
        };
        for (size_t i = 0; i < n; i++)
            if (cull[i].slab_test && !cull[i].unbounded) { mark(cull[i].lo[k]); mark(cull[i].hi[k]); }
    }
    v.n_lights = uint32_t(lights.size());
    v.n_tris = uint32_t(tris.size());
    v.n_obj_tris = uint32_t(n_obj_tris);
    v.has_medium = s->media.empty() ? 0 : 1;
    v.medium_kind = 0;
    v.absorption = v.scattering = 0.0;
    if (!s->media.empty()) {   // only media[0] is used (src/renderer.rs:190)
        v.medium_kind = s->media[0].kind;
        v.absorption = s->media[0].absorption;
        v.scattering = s->media[0].scattering;
        const D3 lo = s->media[0].kind == 1 ? hex_color(0x0000FF) : hex_color(0xD2B48C), hi = s->media[0].kind == 1 ? hex_color(0xFF0000) : lo;
        s->medium_color64[0] = lo.x; s->medium_color64[1] = lo.y; s->medium_color64[2] = lo.z;
        s->medium_color_hi64[0] = hi.x; s->medium_color_hi64[1] = hi.y; s->medium_color_hi64[2] = hi.z;
    }
    for (int k = 0; k < 3; k++) v.env[k] = s->env[k];
    return RPT_OK;
}
// The fp64 kernels' common arguments: the scene, and -- for the camera passes -- camera, frame, tiles and chunking as prepare_render
// laid them out for the fp32 machinery (`a`); cam / prm / a are null for a launch without a camera (photon shooting).
extern "C++" void rpti::fill_args64(rpt_scene* s, const rpt_camera* cam, const rpt_render_params* prm, const RenderArgs* a, rpt64::Args& q) {
    q.sc = s->view64;
    for (int i = 0; i < 3; i++) {
        q.medium_color[i] = s->medium_color64[i];
        q.medium_color_hi[i] = s->medium_color_hi64[i];
    }
    q.cull = uint32_t(s->opt.f64_cull);
    q.surf_batch = uint32_t(s->opt.f64_surf_batch);
    q.group_lights = 0u;
    for (const auto& l : s->lights)
        if (l.kind == int(L_OBJECT) && l.obj.shape.d.kind == RPT_SHAPE_GROUP) q.group_lights = 1u;
    q.mono = rpti::has_monomial(s) ? 1u : 0u;
    q.tree = uint32_t(s->mesh_tree_info64[5]);
    q.mnodes = s->mnodes64;
    q.mleaf = s->mleaf64;
    q.mroot = s->mroot64;
    if (cam) fill_camera64(cam, q.cam);
    if (prm) {
        q.width = prm->width; q.height = prm->height;
        q.max_bounces = prm->max_bounces;
        q.dim = double(std::max(prm->width, prm->height));
    }
    if (a) {
        q.iterations = a->iterations; q.sample_offset = a->sample_offset;
        q.n_owned = a->n_owned; q.tiles_x = a->tiles_x; q.tiles = a->tiles; q.n_items = a->n_items;
        q.chunk_spp = a->chunk_spp; q.n_chunks = a->n_chunks;
        q.pull_batch = a->pull_batch;
        q.seed_mixed = a->seed_mixed;
        q.queue = a->queue;
        q.slab = reinterpret_cast<double*>(a->slab);
    }
    q.counters = nullptr;
}

int rpt_scene_commit(rpt_scene* s, int device) {
    if (!s) return fail(RPT_ERR_INVALID, "null scene");
    if (s->committed) return fail(RPT_ERR_STATE, "scene already committed");
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(RPT_ERR_INVALID, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(RPT_ERR_UNSUPPORTED, std::string("built for gfx950 (MI355X), device is ") + prop.gcnArchName);
    s->n_cus = prop.multiProcessorCount;

    if (s->opt.epsilon_policy == 1)
        if (int rc64 = check_scene64(s)) return rc64;   // (before anything is allocated on the device)
    Flattener f(s);
    int rc = f.flatten_objects();
    if (rc) return rc;
    f.flatten_lights();
    f.fold_shell();
    f.mark_twin_ranges();
    rc = f.build_scene_tree();
    if (rc) return rc;
    f.specialise_scans();
    f.collect_scan_boxes();
    f.group_scans();
    rc = f.upload(device);
    if (rc) return rc;
    if (s->opt.epsilon_policy == 1) {
        rc = build_scene64(s);
        if (rc) { release_device(s); return rc; }
    }
    return RPT_OK;
}

// ---------------------------------------------------------------------------- render
// Tile ownership (host only, no HIP call): 32x32 tiles, tile (tx,ty) belongs to rank (tx+ty) % count.
extern "C" int64_t rpt_shard_tiles(uint32_t width, uint32_t height, uint32_t shard_rank, uint32_t shard_count,
                                   uint32_t* tiles_out, uint64_t capacity) {
    if (shard_count == 0) shard_count = 1;
    if (width == 0 || height == 0 || shard_rank >= shard_count) return fail(RPT_ERR_INVALID, "bad shard arguments");
    uint32_t tiles_x = (width + 31) / 32, tiles_y = (height + 31) / 32;
    int64_t n = 0;
    for (uint32_t ty = 0; ty < tiles_y; ty++)
        for (uint32_t tx = 0; tx < tiles_x; tx++)
            if ((tx + ty) % shard_count == shard_rank) {
                if (tiles_out && uint64_t(n) < capacity) tiles_out[n] = ty * tiles_x + tx;
                n++;
            }
    return n;
}

// Samples per work item.  Small items keep the persistent grid's tail short when a GPU owns only 1/8 of the
// tiles; the value depends on `iterations` alone so that the fp32 partial sums, and hence the image bits, do not
// change with the shard count.  At most 16 chunks per pixel (C3: 16 samples per item, 0.27 GB of partial sums per launch instead of the
// 1.07 GB of 4-sample items; measured with consecutive steps on two streams (tools/chunk_pipelined.py): 25.46 / 25.26 / 25.02 / 24.86 ms per
// step for 4 / 8 / 16 / 32 on the whole frame, 3.31 / 3.34 / 3.40 / 3.51 ms on one rank's shard of an 8-GPU job: an item is also a trip
// through the work-pull code for the whole wave, which some lane needs in 95 % of the trips with 8-sample items and 77 % with 16).
static uint32_t chunk_rule(int64_t opt_chunk_spp, uint32_t iterations, uint32_t min_chunk, uint32_t fixed_chunk) {
    if (fixed_chunk) return fixed_chunk;
    const int64_t chunk = opt_chunk_spp > 0 ? opt_chunk_spp
                                              : std::min<int64_t>(32, std::max<int64_t>(std::max<int64_t>(2, min_chunk), (int64_t(iterations) + 15) / 16));
    return uint32_t(std::min<int64_t>(chunk, iterations));
}
int rpt_render_chunking(uint32_t iterations, uint32_t* chunk_spp, uint32_t* n_chunks) {
    if (iterations == 0) return fail(RPT_ERR_INVALID, "empty render");
    int64_t opt;
    {
        std::lock_guard<std::mutex> lock(g_defaults_mutex);
        opt = g_defaults.chunk_spp;
    }
    const uint32_t c = chunk_rule(opt, iterations, 0, 0);
    if (chunk_spp) *chunk_spp = c;
    if (n_chunks) *n_chunks = (iterations + c - 1) / c;
    return RPT_OK;
}

int rpt_scene_render_chunking(rpt_scene* s, uint32_t iterations, uint32_t* chunk_spp, uint32_t* n_chunks) {
    if (!s) return fail(RPT_ERR_INVALID, "null scene");
    if (iterations == 0) return fail(RPT_ERR_INVALID, "empty render");
    const uint32_t c = chunk_rule(s->opt.chunk_spp, iterations, 0, 0);
    if (chunk_spp) *chunk_spp = c;
    if (n_chunks) *n_chunks = (iterations + c - 1) / c;
    return RPT_OK;
}

// Camera::cast_ray constants (src/camera.rs:66-69), fp64 then rounded once; 1 / max(width, height) of the pixel -> NDC mapping.
// (Renders and the camera hooks form them here.)
static CameraG camera_g(const rpt_camera* cam) {
    CameraG c;
    D3 dir = d3(cam->direction), up = d3(cam->up);
    double dd = 1.0 / std::tan(cam->fov / 2.0);
    D3 right = normalize(cross(dir, up));
    for (int i = 0; i < 3; i++) {
        c.eye[i] = float(cam->eye[i]);
        c.ddir[i] = float(dd * cam->direction[i]);
        c.right[i] = float(comp(right, i));
        c.up[i] = float(cam->up[i]);
    }
    c.aperture = float(cam->aperture);
    c.focal_distance = float(cam->focal_distance);
    return c;
}
static float inv_dim_of(const rpt_render_params* prm) { return float(1.0 / double(std::max(prm->width, prm->height))); }
extern "C++" void rpti::fill_camera64(const rpt_camera* cam, rpt64::Camera& q) {
    const D3 dir = d3(cam->direction), up = d3(cam->up);
    const D3 right = normalize(cross(dir, up));   // src/camera.rs:67-68
    for (int i = 0; i < 3; i++) {
        q.eye[i] = cam->eye[i];
        q.direction[i] = cam->direction[i];
        q.up[i] = cam->up[i];
        q.right[i] = comp(right, i);
    }
    q.d = 1.0 / std::tan(cam->fov / 2.0);
    q.aperture = cam->aperture;
    q.focal_distance = cam->focal_distance;
}

extern "C++" int rpti::prepare_render(rpt_scene* s, hipStream_t st, const rpt_camera* cam, const rpt_render_params* prm, uint32_t iterations,
                         uint64_t seed, uint32_t sample_offset, RenderArgs& a, uint32_t min_chunk, uint32_t fixed_chunk, uint32_t slab_item_bytes,
                         bool launch_set) {
    if (!s || !cam || !prm) return fail(RPT_ERR_INVALID, "null argument");
    if (!s->committed) return fail(RPT_ERR_STATE, "rpt_scene_commit must be called before rendering");
    if (prm->width == 0 || prm->height == 0 || iterations == 0) return fail(RPT_ERR_INVALID, "empty render");
    if (uint64_t(prm->width) * prm->height > (1ull << 31)) return fail(RPT_ERR_INVALID, "image too large");
    uint32_t shard_count = prm->shard_count == 0 ? 1 : prm->shard_count;
    if (prm->shard_rank >= shard_count) return fail(RPT_ERR_INVALID, "shard_rank >= shard_count");
    HIP_TRY(hipSetDevice(s->device));
    if (int rc = rpti::wait_for_move(s, st)) return rc;   // (a scene whose spheres have moved: this pass reads what the move wrote)

    a.sc = s->view;
    a.cam = camera_g(cam);
    a.width = prm->width;
    a.height = prm->height;
    a.inv_dim = inv_dim_of(prm);
    a.max_bounces = prm->max_bounces;
    a.iterations = iterations;
    a.sample_offset = sample_offset;
    a.chunk_spp = chunk_rule(s->opt.chunk_spp, iterations, min_chunk, fixed_chunk);
    a.n_chunks = (iterations + a.chunk_spp - 1) / a.chunk_spp;
    a.seed_mixed = seed_mix(seed);

    // owned tiles
    uint32_t tiles_x = (prm->width + 31) / 32, tiles_y = (prm->height + 31) / 32;
    (void)tiles_y;
    if (s->tk_w != prm->width || s->tk_h != prm->height || s->tk_rank != prm->shard_rank || s->tk_count != shard_count ||
        !s->dev.d_tiles) {
        // Another frame than the last call's: the list this scene already holds for it, else a new one.  Earlier launches may
        // still be reading the lists they were given, so none is written after its upload.
        auto& lists = s->dev.tile_lists;
        size_t at = 0;
        while (at < lists.size() && !(lists[at].w == prm->width && lists[at].h == prm->height && lists[at].rank == prm->shard_rank &&
                                      lists[at].count == shard_count))
            at++;
        if (at == lists.size()) {
            std::vector<uint32_t> tiles(size_t(tiles_x) * tiles_y);
            tiles.resize(size_t(rpt_shard_tiles(prm->width, prm->height, prm->shard_rank, shard_count, tiles.data(),
                                                tiles.size())));
            if (lists.size() >= rpt_scene::Device::kTileLists) {   // full: the least recently used one goes
                size_t old = 0;
                for (size_t i = 1; i < lists.size(); i++)
                    if (lists[i].used < lists[old].used) old = i;
                if (lists[old].ids.get() == s->dev.d_tiles) s->dev.d_tiles = nullptr;
                lists.erase(lists.begin() + old);   // (hipFree: synchronises the device, no launch reads it any more)
                at = lists.size();
            }
            rpt_scene::Device::TileList fresh;
            HIP_TRY(fresh.ids.reserve(std::max<size_t>(tiles.size() * 4, 4)));
            if (!tiles.empty()) HIP_TRY(hipMemcpy(fresh.ids.get(), tiles.data(), tiles.size() * 4, hipMemcpyHostToDevice));
            fresh.w = prm->width; fresh.h = prm->height; fresh.rank = prm->shard_rank; fresh.count = shard_count;
            fresh.n_tiles = uint32_t(tiles.size());
            lists.push_back(std::move(fresh));
        }
        lists[at].used = ++s->tile_clock;
        s->dev.d_tiles = lists[at].ids.get<uint32_t>();
        s->tk_w = prm->width; s->tk_h = prm->height; s->tk_rank = prm->shard_rank; s->tk_count = shard_count;
        s->n_tiles = lists[at].n_tiles;
        s->tiles_x = tiles_x;
    }
    a.tiles = s->dev.d_tiles;
    a.n_tiles = s->n_tiles;
    a.tiles_x = s->tiles_x;
    a.n_owned = a.n_tiles * 1024u;
    uint64_t n_items = uint64_t(a.n_owned) * a.n_chunks;
    if (n_items >= (1ull << 32) - (1ull << 24)) return fail(RPT_ERR_INVALID, "too many work items; raise chunk_spp");
    a.n_items = uint32_t(n_items);
    if (!launch_set) return RPT_OK;   // (what follows configures the render kernels and their scratch)
    size_t slab_bytes = std::max<size_t>(size_t(n_items) * slab_item_bytes, 16);
    // the launch set: the one this stream used last, else the other one
    if (s->dev.sets[s->cur_set].used && s->dev.sets[s->cur_set].stream != st) s->cur_set ^= 1;
    rpt_scene::LaunchSet& ls = s->dev.sets[s->cur_set];
    if (ls.used && ls.stream != st) HIP_TRY(hipStreamWaitEvent(st, ls.done.get(), 0));  // a third stream: wait for the set's last launch
    HIP_TRY(ls.d_slab.reserve(slab_bytes));
    ls.stream = st;
    ls.used = true;
    a.slab = ls.d_slab.get<float>();
    a.queue = ls.d_queue.get<unsigned long long>();
    a.counters = s->opt.counters ? s->dev.d_counters.get<unsigned long long>() : nullptr;
    a.lds_stack = s->view.n_nodes ? 1u : 0u;
    a.defer_lanes = uint32_t(s->opt.defer_lanes);
    a.defer_stop = uint32_t(std::min(s->opt.defer_stop, s->opt.defer_lanes));
    a.walk_leaf_quarters = uint32_t(s->opt.walk_leaf_quarters);
    // Detached shadow queries: in a medium (a path's radiance is linear in its light terms), per-mesh trees, and every
    // light that can be visible has its twin among the scanned records as one range of hit codes.
    a.detach = 0;
    if (s->opt.detach_shadows && s->view.has_medium && bvh_mode(s->view) == 1 && s->view.n_lparts == 0 && s->twins_scanned)
        a.detach = (s->opt.detach_shadows == 2 && s->n_twin_lights <= 3) ? 2u : 1u;
    a.stream_backlog = uint32_t(s->opt.stream_backlog);
    a.stream_contexts = uint32_t(s->opt.stream_contexts);
    a.n_twin_lights = s->n_twin_lights;
    a.stream_scratch = nullptr;   // (render_frame sizes it for the grid)
    a.pull_batch = uint32_t(s->opt.pull_batch);
    a.detach_trigger = uint32_t(s->opt.detach_trigger);
    if (a.detach) {
        a.defer_lanes = uint32_t(s->opt.detach_lanes);
        a.defer_stop = uint32_t(std::min<int64_t>(s->opt.defer_stop, std::min(s->opt.detach_lanes, s->opt.detach_trigger)));   // a session that starts makes progress
    }
    return RPT_OK;
}

// A launch that uses per-scene scratch beyond its launch set (the photon camera pass: candidate lists, overflow
// flag) must not overlap a launch on another stream: wait for whatever the other stream still has in flight.
extern "C++" int rpti::serialize_with_other_streams(rpt_scene* s, hipStream_t st) {
    for (auto& ls : s->dev.sets)
        if (ls.used && ls.stream != st) HIP_TRY(hipStreamWaitEvent(st, ls.done.get(), 0));
    return RPT_OK;
}

extern "C++" int rpti::run_persistent(rpt_scene* s, const rpt_render_params* prm, const RenderArgs& a, double* d_out, hipStream_t st,
                         const PersistentLaunch& pl) {
    const int k = s->dev.sets[0].d_queue.get() == a.queue ? 0 : 1;
    rpt_scene::LaunchSet& mine = s->dev.sets[k];
    rpt_scene::LaunchSet& other = s->dev.sets[k ^ 1];
    // Two launches that become ready at the same moment would share the CUs block by block, and the half of each
    // grid that finds no room would start after everything else has drained (measured: 31.3 instead of 30.0 ms per
    // step).  So a launch on the second stream is released only once the first stream has reached its kernel: the
    // grids then follow each other, the later one filling the CUs as the blocks of the earlier one retire.
    if (other.used && other.stream != st) HIP_TRY(hipStreamWaitEvent(st, other.launched.get(), 0));
    HIP_TRY(hipMemsetAsync(a.queue, 0, 8, st));
    if (a.counters) HIP_TRY(hipMemsetAsync(a.counters, 0, 640, st));
    uint32_t shard_count = prm->shard_count == 0 ? 1 : prm->shard_count;
    if (shard_count > 1 && pl.clear_sharded) HIP_TRY(hipMemsetAsync(d_out, 0, size_t(prm->width) * prm->height * 24, st));
    if (a.n_items) {
        uint64_t want = pl.wave_items ? (uint64_t(a.n_items) + 3) / 4 : (uint64_t(a.n_items) + 255) / 256;
        int n_blocks = int(std::min<uint64_t>(uint64_t(s->n_cus) * std::max(pl.blocks_per_cu, 1), want));
        if (s->opt.max_blocks > 0) n_blocks = int(std::min<int64_t>(n_blocks, s->opt.max_blocks));   // (scratch per wave is sized for the uncapped grid)
        s->last_blocks = n_blocks;
        // indexed_start: every wave of the grid takes the batch with its own index first (render_kernel's work
        // pull), so the counter starts behind those batches
        if (pl.indexed_start) HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)a.queue, int(uint32_t(n_blocks) * 4u * 64u), 1, st));
        const rpti::Event* ev = nullptr;
        if (s->opt.timing) {
            const size_t slot = s->ev_count % rpt_scene::kTimedLaunches;
            while (s->dev.evs.size() < 3 * (slot + 1)) {
                rpti::Event e;
                HIP_TRY(e.create());
                s->dev.evs.push_back(std::move(e));
            }
            ev = &s->dev.evs[3 * slot];
            HIP_TRY(hipEventRecord(ev[0].get(), st));
        }
        HIP_TRY(hipEventRecord(mine.launched.get(), st));
        HIP_TRY(pl.launch(a, n_blocks, st));
        if (ev) HIP_TRY(hipEventRecord(ev[1].get(), st));
        if (pl.resolve) HIP_TRY(pl.resolve(std::pow(2.0, prm->exposure_value), d_out, st));
        else HIP_TRY(launch_resolve(a, std::pow(2.0, prm->exposure_value), d_out, st));
        if (ev) {
            HIP_TRY(hipEventRecord(ev[2].get(), st));
            s->ev_count++;
        }
    }
    HIP_TRY(hipEventRecord(mine.done.get(), st));
    return RPT_OK;
}
// ---------------------------------------------------------------------------- scan JIT
// The scan flavours' render kernel compiled for one scene's record counts.  What a scan knows before it
// reads a record -- the counts per kind, the shell, the y-rotation masks, the tail cull -- is fixed at commit and costs the generic
// kernel a chain of scalar loads, waits, compares and branches per kind, twice per wave trip.  hiprtc (opened with dlopen: no link
// dependency) compiles kernels.hip with these as constants (device_core.h, ScanShapeK); record VALUES stay data, so scenes of one shape
// share one code object.  Everything that goes wrong -- library absent, sources absent, compile or load error, more registers than the
// AOT twin -- leaves the scene on the AOT kernel and is said by rpt_scan_jit_info.
extern "C++" {
namespace rpti {
bool scan_shape_of(const SceneView& v, ScanShape* out, std::string* why) {
    if (why) why->clear();
    const char* w = nullptr;
    if (v.n_lparts) w = "a group is a light (GROUPS)";
    else if (v.n_mono) w = "the scene has monomial surfaces (MONO)";
    else if (v.scene_bvh || v.n_nodes) w = "the scene has a tree (BVH != 0)";
    if (w) { if (why) *why = w; return false; }
    *out = ScanShape{v.n_sph, v.n_cub, v.n_pln, v.n_aabb, v.n_rect_x, v.n_rect_y, v.n_rect_z, v.n_tri, v.has_shell ? 1u : 0u,
                     v.scan_cull ? 1u : 0u, v.has_medium ? 1u : 0u, v.sph_yrot, v.cub_yrot};
    return true;
}
// The constants in ScanShapeK's order (device_core.h), as they stand behind "#define RPT_SCAN_SHAPE".
std::string scan_shape_constants(const ScanShape& h) {
    char b[256];
    std::snprintf(b, sizeof b, "%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,0x%llxull,0x%llxull", h.n_sph, h.n_cub, h.n_pln, h.n_aabb, h.n_rect_x, h.n_rect_y,
                  h.n_rect_z, h.n_tri, h.has_shell, h.scan_cull, (unsigned long long)h.sph_yrot, (unsigned long long)h.cub_yrot);
    return b;
}
std::string scan_shape_string(const ScanShape& h) { return scan_shape_constants(h) + (h.medium ? ";medium=1" : ";medium=0"); }
std::string scan_jit_kernel_name(const ScanShape& h) {
    return std::string("rptg::render_kernel<") + (h.medium ? "true" : "false") + ", 0, false, false, 0, false>";
}
std::string scan_jit_program(const ScanShape& h) {
    return "#define RPT_SCAN_SHAPE " + scan_shape_constants(h) + "\n#include \"kernels.hip\"\n";
}
// ---- the structure block
// The groups that passed the acceptance rule on C3 (profiles/r11/scan_jit_structure.txt).  SS_SMALL (the medium's kind, no HDRI) gains
// 0.09 - 0.11 ms of 15.1, within three times the run-to-run range: it stays a switch.
static constexpr uint32_t kStructDefaultGroups = SS_ALL & ~SS_SMALL;
uint32_t scan_struct_default_groups() {
    const char* env = std::getenv("RPT_SCAN_STRUCT_GROUPS");
    if (!env || !*env) return kStructDefaultGroups;
    char* end = nullptr;
    const unsigned long v = std::strtoul(env, &end, 0);
    return (end && *end == 0) ? uint32_t(v) & SS_ALL : kStructDefaultGroups;
}
SceneStruct scan_struct_of(uint32_t groups, const std::vector<Light>& lights, const std::vector<LightXf>& lxf, size_t n_ltris,
                           const std::vector<Material>& mats, const std::vector<AabbScan>& aabb, uint32_t medium_kind, bool hdri) {
    SceneStruct t{};
    groups &= SS_ALL;
    if (lights.size() > kStructLights) groups &= ~SS_LIGHTS;                     // the light loop reads them from the view
    if (mats.size() > kLdsMats || n_ltris > kLdsLtris) groups &= ~SS_TABLES;     // a table stays in global memory
    if (aabb.size() / 2 > kStructPairs) groups &= ~SS_PAIRS;
    for (const Light& L : lights)   // (a group light is outside the JIT's scope altogether: scan_shape_of)
        if (L.kind == L_OBJECT && (L.shape == LS_GROUP || L.xf >= lxf.size())) groups &= ~SS_LIGHTS;
    t.groups = groups;
    if (groups & SS_LIGHTS) {
        t.n_lights = uint32_t(lights.size());
        for (size_t i = 0; i < lights.size(); i++) {
            const Light& L = lights[i];
            uint32_t w = L.kind & 3u;
            if (L.kind == L_OBJECT) {
                const bool range = L.twin_lo <= L.twin_hi;
                w |= (L.shape & 3u) << 2 | (lxf[L.xf].nrm[1].w != 0.f ? 16u : 0u) | (L.twin_object >= 0 ? 32u : 0u) | (range ? 64u : 0u);
                if (range) { t.twin_lo[i] = L.twin_lo; t.twin_hi[i] = L.twin_hi; }
            }
            t.light[i] = w;
        }
    }
    if (groups & SS_MATS)
        for (const Material& m : mats) t.mats |= 1u << (bits_u(m.params.x) & 3u);
    if (groups & SS_SMALL) { t.medium_kind = medium_kind; t.hdri = hdri ? 1u : 0u; }
    if (groups & SS_PAIRS)
        for (size_t i = 0; i + 1 < aabb.size(); i += 2) t.pairs |= uint64_t(bits_u(aabb[i].hi.w) & 7u) << (3 * (i / 2));
    return t;
}
// The constants in SceneStructK's order (device_core.h), as they stand behind "#define RPT_SCENE_STRUCT".
std::string scan_struct_constants(const SceneStruct& t) {
    std::string o = std::to_string(t.groups) + "," + std::to_string(t.n_lights);
    for (const uint32_t* f : {t.light, t.twin_lo, t.twin_hi})
        for (int i = 0; i < 4; i++) o += "," + std::to_string(f[i]) + "u";
    char b[64];
    std::snprintf(b, sizeof b, ",%u,%u,%u,0x%llxull", t.mats, t.medium_kind, t.hdri, (unsigned long long)t.pairs);
    return o + b;
}
std::string scan_struct_string(const SceneStruct& t) {
    static const char* const group_names[5] = {"lights", "tables", "mats", "small", "pairs"};
    static const char* const kinds[4] = {"point", "ambient", "directional", "object"};
    static const char* const shapes[4] = {"sphere", "cube", "group", "mesh"};
    std::string o = "groups=";
    for (int g = 0; g < 5; g++)
        if (t.groups & (1u << g)) o += std::string(o.back() == '=' ? "" : "+") + group_names[g];
    if (!t.groups) o += "none";
    o += ";lights=";
    if (!(t.groups & SS_LIGHTS)) o += "view";
    else {
        o += std::to_string(t.n_lights);
        for (uint32_t i = 0; i < t.n_lights; i++) {
            const uint32_t w = t.light[i];
            o += std::string(i ? "|" : ":") + kinds[w & 3u];
            if ((w & 3u) != L_OBJECT) continue;
            o += std::string("/") + shapes[(w >> 2) & 3u] + ((w & 16u) ? "/xf" : "") + ((w & 32u) ? "/twin" : "");
            char b[48];
            std::snprintf(b, sizeof b, "/%x-%x", t.twin_lo[i], t.twin_hi[i]);
            if (w & 64u) o += b;
        }
    }
    char b[96];
    if (t.groups & SS_MATS) { std::snprintf(b, sizeof b, ";mats=0x%x", t.mats); o += b; } else o += ";mats=view";
    if (t.groups & SS_SMALL) { std::snprintf(b, sizeof b, ";medium_kind=%u;hdri=%u", t.medium_kind, t.hdri); o += b; } else o += ";medium_kind=view;hdri=view";
    if (t.groups & SS_PAIRS) { std::snprintf(b, sizeof b, ";pairs=0x%llx", (unsigned long long)t.pairs); o += b; } else o += ";pairs=view";
    return o;
}
std::string scan_jit_program(const ScanShape& h, const SceneStruct& t) {
    // The last line names the instantiation: the medium is part of the shape and of the kernel's name but of neither block, and the cache
    // key is taken over this text -- a scene in fog and one without, alike in every count, must not share a code object.
    return "#define RPT_SCAN_SHAPE " + scan_shape_constants(h) + "\n#define RPT_SCENE_STRUCT " + scan_struct_constants(t) + "\n#include \"kernels.hip\"\n// " +
           scan_jit_kernel_name(h) + "\n";
}
const std::vector<std::string>& scan_jit_options() {   // the library's own device flags (__graft_entry__.FLAGS)
    static const std::vector<std::string> o = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize"};
    return o;
}
// kernels.hip and every file it includes with quotes, transitively, as read from `dir`: (include name, contents) in the order found.
// They are handed to the compiler from memory, so what is hashed is what is compiled.
bool scan_jit_sources(const std::string& dir, std::vector<std::pair<std::string, std::string>>* out, std::string* why) {
    out->clear();
    std::vector<std::string> todo = {"kernels.hip"};
    while (!todo.empty()) {
        const std::string name = todo.back();
        todo.pop_back();
        bool have = false;
        for (auto& f : *out) have = have || f.first == name;
        if (have) continue;
        FILE* f = std::fopen((dir + "/" + name).c_str(), "rb");
        if (!f) { *why = "source not found: " + dir + "/" + name; return false; }
        std::string text;
        char buf[65536];
        for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, n);
        std::fclose(f);
        for (size_t p = 0; (p = text.find("#include \"", p)) != std::string::npos;) {
            p += 10;
            const size_t e = text.find('"', p);
            if (e == std::string::npos) break;
            const std::string inc = text.substr(p, e - p);
            if (inc.find('/') == std::string::npos) todo.push_back(inc);   // (the program needs no file outside csrc/)
            p = e;
        }
        out->emplace_back(name, std::move(text));
    }
    return true;
}
// 128 bits (two FNV-1a streams with different offsets) over the exact program text, every source as read, the options and the hiprtc
// version: a cache key, not a signature.
std::string scan_jit_key(const std::string& program, const std::vector<std::pair<std::string, std::string>>& sources,
                         const std::vector<std::string>& options, int rtc_major, int rtc_minor) {
    uint64_t h0 = 0xCBF29CE484222325ULL, h1 = 0x84222325CBF29CE4ULL;
    auto eat = [&](const std::string& s) {
        const uint64_t n = s.size();
        for (int i = 0; i < 8; i++) { h0 = (h0 ^ ((n >> (8 * i)) & 255u)) * 0x100000001B3ULL; h1 = (h1 ^ ((n >> (8 * i)) & 255u)) * 0x100000001B3ULL; }
        for (unsigned char c : s) { h0 = (h0 ^ c) * 0x100000001B3ULL; h1 = (h1 ^ c) * 0x100000001B3ULL; h1 ^= h1 >> 29; }
    };
    eat(program);
    for (auto& f : sources) { eat(f.first); eat(f.second); }
    for (auto& o : options) eat(o);
    eat("hiprtc " + std::to_string(rtc_major) + "." + std::to_string(rtc_minor));
    char b[40];
    std::snprintf(b, sizeof b, "%016llx%016llx", (unsigned long long)h0, (unsigned long long)h1);
    return b;
}
// VGPRs and scratch bytes per lane of the (one) kernel of a code object, from its metadata note: the MessagePack map entries
// ".vgpr_count" and ".private_segment_fixed_size" (a string key followed by an unsigned integer).
bool scan_jit_resources(const std::vector<char>& code, int* vgprs, int* scratch) {
    auto find = [&](const char* key, int* out) {
        const size_t kl = std::strlen(key);
        for (size_t i = 0; i + kl + 1 <= code.size(); i++) {
            if (std::memcmp(code.data() + i, key, kl) != 0) continue;
            const unsigned char* p = reinterpret_cast<const unsigned char*>(code.data()) + i + kl;
            const size_t left = code.size() - i - kl;
            if (left >= 1 && p[0] < 0x80) { *out = p[0]; return true; }
            if (left >= 2 && p[0] == 0xCC) { *out = p[1]; return true; }
            if (left >= 3 && p[0] == 0xCD) { *out = (p[1] << 8) | p[2]; return true; }
            if (left >= 5 && p[0] == 0xCE) { *out = int((uint32_t(p[1]) << 24) | (p[2] << 16) | (p[3] << 8) | p[4]); return true; }
        }
        return false;
    };
    return find(".vgpr_count", vgprs) && find(".private_segment_fixed_size", scratch);
}

namespace {
struct Hiprtc {   // the entry points of libhiprtc this file uses (signatures of hip/hiprtc.h; the header is not needed)
    void* lib = nullptr;
    std::string path;
    int major = 0, minor = 0;
    int (*version)(int*, int*) = nullptr;
    int (*create)(void**, const char*, const char*, int, const char* const*, const char* const*) = nullptr;
    int (*destroy)(void**) = nullptr;
    int (*add_name)(void*, const char*) = nullptr;
    int (*compile)(void*, int, const char* const*) = nullptr;
    int (*lowered)(void*, const char*, const char**) = nullptr;
    int (*log_size)(void*, size_t*) = nullptr;
    int (*log)(void*, char*) = nullptr;
    int (*code_size)(void*, size_t*) = nullptr;
    int (*code)(void*, char*) = nullptr;
};
struct HipModules {   // the module entry points of the HIP runtime this library is linked to, looked up by name: a build that stubs the
    bool looked = false, ok = false;   // runtime (tests/host) has none of them and simply has no JIT
    hipError_t (*load_data)(hipModule_t*, const void*) = nullptr;
    hipError_t (*get_function)(hipFunction_t*, hipModule_t, const char*) = nullptr;
    hipError_t (*launch)(hipFunction_t, unsigned, unsigned, unsigned, unsigned, unsigned, unsigned, unsigned, hipStream_t, void**, void**) = nullptr;
};
struct JitObject {
    std::vector<char> code;
    std::string lowered;
    int vgprs = 0, scratch = 0;
    double compile_ms = 0;
    std::string rejected;   // not empty: compiled (or failed to) and not to be used, why
    std::unordered_map<int, hipFunction_t> fn;   // per device; modules stay loaded for the life of the process
};
std::mutex g_jit_mutex;   // everything below
std::unordered_map<std::string, Hiprtc> g_hiprtc;   // by path (RPT_HIPRTC_LIB may change between scenes)
HipModules g_modules;
std::unordered_map<std::string, JitObject> g_jit_objects;   // by key
uint64_t g_jit_compiles = 0;

const Hiprtc* hiprtc_open(std::string* why) {
    const char* env = std::getenv("RPT_HIPRTC_LIB");
    const std::vector<std::string> paths = env && *env ? std::vector<std::string>{env} : std::vector<std::string>{"/opt/rocm/lib/libhiprtc.so", "libhiprtc.so"};   // (the compiler the library was built with first)
    for (const std::string& path : paths) {
        auto it = g_hiprtc.find(path);
        if (it != g_hiprtc.end()) { if (it->second.lib) return &it->second; continue; }
        Hiprtc& h = g_hiprtc[path];
        void* lib = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
        if (!lib) continue;
        bool ok = true;
        auto sym = [&](auto& fn, const char* name) { fn = reinterpret_cast<std::remove_reference_t<decltype(fn)>>(dlsym(lib, name)); ok = ok && fn; };
        sym(h.version, "hiprtcVersion"); sym(h.create, "hiprtcCreateProgram"); sym(h.destroy, "hiprtcDestroyProgram");
        sym(h.add_name, "hiprtcAddNameExpression"); sym(h.compile, "hiprtcCompileProgram"); sym(h.lowered, "hiprtcGetLoweredName");
        sym(h.log_size, "hiprtcGetProgramLogSize"); sym(h.log, "hiprtcGetProgramLog"); sym(h.code_size, "hiprtcGetCodeSize");
        sym(h.code, "hiprtcGetCode");
        if (!ok || h.version(&h.major, &h.minor) != 0) { dlclose(lib); continue; }
        h.lib = lib;
        h.path = path;
        return &h;
    }
    *why = "hiprtc not available (" + paths[0] + ")";
    return nullptr;
}
const HipModules& hip_modules() {
    HipModules& m = g_modules;
    if (m.looked) return m;
    m.looked = true;
    Dl_info di{};
    if (!dladdr(reinterpret_cast<void*>(&hipGetDeviceCount), &di) || !di.dli_fname) return m;
    void* lib = dlopen(di.dli_fname, RTLD_NOW | RTLD_NOLOAD);
    if (!lib) return m;
    m.load_data = reinterpret_cast<decltype(m.load_data)>(dlsym(lib, "hipModuleLoadData"));
    m.get_function = reinterpret_cast<decltype(m.get_function)>(dlsym(lib, "hipModuleGetFunction"));
    m.launch = reinterpret_cast<decltype(m.launch)>(dlsym(lib, "hipModuleLaunchKernel"));
    m.ok = m.load_data && m.get_function && m.launch;
    return m;
}
std::string jit_source_dir() {
    if (const char* env = std::getenv("RPT_JIT_SRC")) if (*env) return env;
    Dl_info di{};
    if (!dladdr(reinterpret_cast<void*>(&rpt_last_error), &di) || !di.dli_fname) return "";
    const std::string lib = di.dli_fname;
    const size_t slash = lib.rfind('/');
    return (slash == std::string::npos ? std::string(".") : lib.substr(0, slash)) + "/csrc";
}
std::string jit_cache_dir() {
    if (const char* env = std::getenv("RPT_JIT_CACHE")) if (*env) return env;
    const char* home = std::getenv("HOME");
    return home && *home ? std::string(home) + "/.cache/rpt_amd/jit" : std::string();
}
uint64_t fnv_bytes(const void* p, size_t n, uint64_t h = 0xCBF29CE484222325ULL) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001B3ULL;
    return h;
}
}  // namespace

// A cache file: "RPTJIT01", code bytes, name bytes, FNV-1a of name + code (three u64), the lowered name, the code object.
bool scan_jit_cache_read(const std::string& path, std::vector<char>* code, std::string* lowered, std::string* why) {
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) { *why = "no cache file"; return false; }
    char magic[8];
    uint64_t hd[3] = {0, 0, 0};
    bool ok = std::fread(magic, 1, 8, f) == 8 && std::memcmp(magic, "RPTJIT01", 8) == 0 && std::fread(hd, 8, 3, f) == 3 && hd[0] > 0 &&
              hd[0] < (uint64_t(1) << 28) && hd[1] > 0 && hd[1] < 4096;
    if (ok) {
        lowered->resize(size_t(hd[1]));
        code->resize(size_t(hd[0]));
        ok = std::fread(&(*lowered)[0], 1, lowered->size(), f) == lowered->size() && std::fread(code->data(), 1, code->size(), f) == code->size() &&
             fnv_bytes(code->data(), code->size(), fnv_bytes(lowered->data(), lowered->size())) == hd[2];
    }
    std::fclose(f);
    if (!ok) *why = "cache file truncated or damaged";
    return ok;
}
bool scan_jit_cache_write(const std::string& dir, const std::string& path, const std::vector<char>& code, const std::string& lowered) {
    std::error_code ec;
    std::filesystem::create_directories(dir, ec);
    static std::atomic<unsigned> serial{0};
    const std::string tmp = path + ".tmp." + std::to_string(uint64_t(getpid())) + "." + std::to_string(serial++);   // (the ranks of one job write the same file at once)
    FILE* f = std::fopen(tmp.c_str(), "wb");
    if (!f) return false;
    const uint64_t hd[3] = {code.size(), lowered.size(), fnv_bytes(code.data(), code.size(), fnv_bytes(lowered.data(), lowered.size()))};
    bool ok = std::fwrite("RPTJIT01", 1, 8, f) == 8 && std::fwrite(hd, 8, 3, f) == 3 && std::fwrite(lowered.data(), 1, lowered.size(), f) == lowered.size() &&
              std::fwrite(code.data(), 1, code.size(), f) == code.size();
    ok = (std::fclose(f) == 0) && ok;
    if (ok) ok = std::rename(tmp.c_str(), path.c_str()) == 0;
    if (!ok) std::remove(tmp.c_str());
    return ok;
}
// One compile, in this process.  `rtc` null: the library is opened here (tests/host).
bool scan_jit_compile(const ScanShape& shape, const std::vector<std::pair<std::string, std::string>>& sources, std::vector<char>* code,
                      std::string* lowered, double* ms, std::string* why) {
    return scan_jit_compile(shape, nullptr, sources, code, lowered, ms, why);
}
// ... `structure` null: the shape block alone.
bool scan_jit_compile(const ScanShape& shape, const SceneStruct* structure, const std::vector<std::pair<std::string, std::string>>& sources,
                      std::vector<char>* code, std::string* lowered, double* ms, std::string* why) {
    std::string w;
    const Hiprtc* rtc = hiprtc_open(&w);
    if (!rtc) { *why = w; return false; }
    const std::string program = structure ? scan_jit_program(shape, *structure) : scan_jit_program(shape), name = scan_jit_kernel_name(shape);
    std::vector<const char*> texts, names, opts;
    for (auto& f : sources) { names.push_back(f.first.c_str()); texts.push_back(f.second.c_str()); }
    for (auto& o : scan_jit_options()) opts.push_back(o.c_str());
    void* prog = nullptr;
    if (rtc->create(&prog, program.c_str(), "rpt_scan_jit.hip", int(texts.size()), texts.data(), names.data()) != 0) { *why = "hiprtcCreateProgram failed"; return false; }
    const auto t0 = std::chrono::steady_clock::now();
    bool ok = rtc->add_name(prog, name.c_str()) == 0;
    if (!ok) *why = "hiprtcAddNameExpression failed";
    if (ok && rtc->compile(prog, int(opts.size()), opts.data()) != 0) {
        ok = false;
        size_t n = 0;
        std::string log;
        if (rtc->log_size(prog, &n) == 0 && n > 1) { log.resize(n); rtc->log(prog, &log[0]); }
        *why = "compile error: " + log.substr(0, 600);
    }
    *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    const char* low = nullptr;
    size_t n = 0;
    if (ok && (rtc->lowered(prog, name.c_str(), &low) != 0 || !low)) { ok = false; *why = "no lowered name for " + name; }
    if (ok) *lowered = low;
    if (ok && (rtc->code_size(prog, &n) != 0 || n == 0)) { ok = false; *why = "empty code object"; }
    if (ok) { code->resize(n); if (rtc->code(prog, code->data()) != 0) { ok = false; *why = "hiprtcGetCode failed"; } }
    rtc->destroy(&prog);
    return ok;
}
}  // namespace rpti

// The specialised function for this launch, or null: the AOT kernel.  Called with the scene's device current.
static hipFunction_t scan_jit_function(rpt_scene* s, const RenderArgs& a) {
    using namespace rpti;
    ScanJit& j = s->jit;
    if (s->opt.scan_jit == 0 || a.counters) return nullptr;   // (the counters build is a flavour of its own)
    if (j.fn) return j.fn;
    if (j.state == RPT_SCAN_JIT_FALLBACK || j.state == RPT_SCAN_JIT_OUT_OF_SCOPE) return nullptr;
    std::lock_guard<std::mutex> lock(g_jit_mutex);
    auto give_up = [&](int state, const std::string& why) { j.state = state; j.reason = why; return nullptr; };
    if (!j.probed) {   // once per scene: shape, sources, key, and a look into both caches
        j.probed = true;
        ScanShape shape;
        std::string why;
        if (!scan_shape_of(s->view, &shape, &why)) return give_up(RPT_SCAN_JIT_OUT_OF_SCOPE, why);
        j.shape = shape;
        j.shape_text = scan_shape_string(shape);
        if (!scan_render_info) return give_up(RPT_SCAN_JIT_FALLBACK, "this build has no AOT twin to compare with");
        if (!hip_modules().ok) return give_up(RPT_SCAN_JIT_FALLBACK, "the HIP runtime has no module entry points");
        const Hiprtc* rtc = hiprtc_open(&why);
        if (!rtc) return give_up(RPT_SCAN_JIT_FALLBACK, why);
        if (!scan_jit_sources(jit_source_dir(), &j.sources, &why)) return give_up(RPT_SCAN_JIT_FALLBACK, why);
        j.key = scan_jit_key(scan_jit_program(shape, j.structure), j.sources, scan_jit_options(), rtc->major, rtc->minor);
        j.compiler = "hiprtc " + std::to_string(rtc->major) + "." + std::to_string(rtc->minor) + " (" + rtc->path + ")";
        int aot_scratch = 0;
        if (scan_render_info(shape.medium != 0, &j.aot_vgprs, &aot_scratch, &j.lds) != hipSuccess || j.aot_vgprs <= 0)
            return give_up(RPT_SCAN_JIT_FALLBACK, "the AOT twin's registers are unknown");
    }
    const int aot_vgprs = j.aot_vgprs;
    auto it = g_jit_objects.find(j.key);
    int cache = RPT_SCAN_JIT_CACHE_MEMORY;
    const std::string dir = jit_cache_dir(), path = dir.empty() ? std::string() : dir + "/" + j.key + ".co";
    std::string note;
    if (it == g_jit_objects.end() && !path.empty()) {
        JitObject o;
        std::string why;
        if (scan_jit_cache_read(path, &o.code, &o.lowered, &why) && scan_jit_resources(o.code, &o.vgprs, &o.scratch)) {
            it = g_jit_objects.emplace(j.key, std::move(o)).first;
            cache = RPT_SCAN_JIT_CACHE_DISK;
        } else if (why != "no cache file") {
            std::remove(path.c_str());   // a file that does not load is discarded and compiled again
            note = "cache file discarded (" + (why.empty() ? std::string("no resource note") : why) + "); ";
        }
    }
    if (it == g_jit_objects.end()) {
        const uint64_t samples = uint64_t(a.n_owned) * a.iterations;
        if (s->opt.scan_jit == 1 && samples < (uint64_t(1) << 27)) {   // (not final: a larger launch compiles)
            j.state = RPT_SCAN_JIT_IDLE;
            j.reason = note + "no cached code object, and the launch is below the compile threshold of 2^27 camera samples";
            return nullptr;
        }
        JitObject o;
        std::string why;
        g_jit_compiles++;
        if (!scan_jit_compile(j.shape, &j.structure, j.sources, &o.code, &o.lowered, &o.compile_ms, &why)) o.rejected = why;
        else if (!scan_jit_resources(o.code, &o.vgprs, &o.scratch)) o.rejected = "no resource note in the code object";
        else if (!path.empty()) (void)scan_jit_cache_write(dir, path, o.code, o.lowered);   // (an unwritable directory: memory only)
        it = g_jit_objects.emplace(j.key, std::move(o)).first;
        cache = RPT_SCAN_JIT_CACHE_MISS;
    }
    JitObject& o = it->second;
    j.cache = cache;
    j.compile_ms = cache == RPT_SCAN_JIT_CACHE_MISS ? o.compile_ms : 0.0;
    j.vgprs = o.vgprs;
    j.scratch = o.scratch;
    if (!o.rejected.empty()) return give_up(RPT_SCAN_JIT_FALLBACK, note + o.rejected);
    if (o.vgprs > aot_vgprs)
        return give_up(RPT_SCAN_JIT_FALLBACK, note + std::to_string(o.vgprs) + " VGPRs against the AOT kernel's " + std::to_string(aot_vgprs));
    auto fn = o.fn.find(s->device);
    if (fn == o.fn.end()) {
        hipModule_t mod = nullptr;
        hipFunction_t f = nullptr;
        hipError_t e = hip_modules().load_data(&mod, o.code.data());
        if (e == hipSuccess) e = hip_modules().get_function(&f, mod, o.lowered.c_str());
        if (e != hipSuccess || !f) {
            if (cache == RPT_SCAN_JIT_CACHE_DISK) { std::remove(path.c_str()); g_jit_objects.erase(it); }
            return give_up(RPT_SCAN_JIT_FALLBACK, note + "load error: " + hipGetErrorString(e));
        }
        fn = o.fn.emplace(s->device, f).first;
    }
    j.fn = fn->second;
    j.state = RPT_SCAN_JIT_ACTIVE;
    j.reason = note + j.compiler;
    return j.fn;
}
static hipError_t launch_render_jit(rpt_scene* s, hipFunction_t fn, const RenderArgs& a, int n_blocks, hipStream_t stream) {
    size_t size = sizeof(RenderArgs);
    void* extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, const_cast<RenderArgs*>(&a), HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
    s->jit.launches++;
    return rpti::hip_modules().launch(fn, unsigned(n_blocks), 1, 1, 256, 1, 1, unsigned(s->jit.lds), stream, nullptr, extra);
}
}  // extern "C++"

extern "C++" double* rpti::scratch_out(rpt_scene* s, size_t bytes) {
    return s->dev.d_out.reserve(bytes) == hipSuccess ? s->dev.d_out.get<double>() : nullptr;
}
extern "C++" int rpti::fetch_counters(rpt_scene* s, const RenderArgs& a) {
    std::memset(s->last_counters, 0, sizeof(s->last_counters));
    std::memset(s->last_cull, 0, sizeof(s->last_cull));
    if (a.counters) {
        HIP_TRY(hipMemcpy(s->last_counters, a.counters, 512, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(s->last_cull, a.counters + 64, sizeof(s->last_cull), hipMemcpyDeviceToHost));
        s->last_counters[4] = s->last_counters[1] * s->prims_per_ray;
    }
    return RPT_OK;
}
// The reference-epsilon kernels' counters, after the stream has been synchronised.
static int fetch_counters64(rpt_scene* s, const RenderArgs& a) {
    std::memset(s->last_counters, 0, sizeof(s->last_counters));
    HIP_TRY(hipMemcpy(s->last_counters64, a.counters, sizeof(s->last_counters64), hipMemcpyDeviceToHost));
    s->last_counters[0] = s->last_counters64[6];   // rpt_get_counters: samples, rays, vertices
    s->last_counters[1] = s->last_counters64[0];
    s->last_counters[2] = s->last_counters64[7];
    s->last_counters[3] = s->last_counters64[10];   // wave-level loop trips
    for (int i = 0; i < 48; i++) s->last_counters[8 + i] = s->last_counters64[16 + i];   // rpt_debug_section_counters
    return RPT_OK;
}

// ---- rpt_render_sample_tiles*: the kernels of a full render on a caller's tile list.
// The list replaces the scene's in the launch arguments only: the scene's cached d_tiles keeps the full frame's list, which a launch
// on the other launch set may still be reading.  The slab prepare_render reserved is the full frame's: no smaller than the list's.
static int use_tile_list(RenderArgs& a, const uint32_t* d_tiles, uint32_t n_tiles) {
    if (n_tiles > a.n_tiles) return fail(RPT_ERR_INVALID, "more tiles listed than the frame has");
    a.tiles = d_tiles;
    a.n_tiles = n_tiles;
    a.n_owned = n_tiles * 1024u;
    const uint64_t n_items = uint64_t(a.n_owned) * a.n_chunks;
    if (n_items >= (1ull << 32) - (1ull << 24)) return fail(RPT_ERR_INVALID, "too many work items; raise chunk_spp");
    a.n_items = uint32_t(n_items);
    return RPT_OK;
}

// Renderer::sample, one frame: a persistent grid over (pixel, chunk) items, one launch set per stream, the slab resolved into d_out.
// The mode the scene was committed in is asked here and nowhere else: the reference-epsilon mode runs the same launch scheme with
// an fp64 slab and its own kernels, occupancy and counters.  d_out null: the scene's cached frame (the host entry point), reserved
// where it always was, after prepare_render.
static int render_frame(rpt_scene* s, const rpt_camera* cam, const rpt_render_params* prm, uint32_t iterations, uint64_t seed,
                        uint32_t sample_offset, double* d_out, hipStream_t st, const uint32_t* d_tiles = nullptr, uint32_t n_tiles = 0) {
    const bool f64 = s && s->dev.arena64;
    RenderArgs a{};   // (tiles, sharding, chunking, launch sets and argument checks are the same in both modes)
    int rc = rpti::prepare_render(s, st, cam, prm, iterations, seed, sample_offset, a, 0, 0, f64 ? 32 : 16);
    if (rc) return rc;
    if (!d_out && !(d_out = rpti::scratch_out(s, size_t(prm->width) * prm->height * 24))) return fail(RPT_ERR_DEVICE, "out of device memory");
    if (d_tiles)   // rpt_render_sample_tiles*: the caller's list in place of the scene's
        if ((rc = use_tile_list(a, d_tiles, n_tiles))) return rc;
    rpt64::Args q{};
    if (f64) {
        rpti::fill_args64(s, cam, prm, &a, q);
        q.counters = a.counters;
    }
    rpti::PersistentLaunch pl;
    pl.indexed_start = true;
    pl.blocks_per_cu = int(s->opt.blocks_per_cu);
    if (pl.blocks_per_cu <= 0) {
        int bpc = 0;
        if (f64) HIP_TRY(render_f64_occupancy(q.sc.has_medium != 0, &bpc));
        else HIP_TRY(render_occupancy(a.sc.has_medium != 0, bvh_mode(a.sc), &bpc, int(a.detach)));
        pl.blocks_per_cu = std::max(bpc, 1);
    }
    if (f64) {
        pl.launch = [&q](const RenderArgs&, int nb, hipStream_t stream) { return launch_render_f64(q, nb, stream); };
        pl.resolve = [&q](double scale, double* out, hipStream_t stream) { return launch_resolve_f64(q, scale, out, stream); };
    } else {
        if (a.detach == 2) {   // the waves' rings and parked paths: per launch set, like the slab (two launches may be in flight)
            rpt_scene::LaunchSet& ls = s->dev.sets[s->dev.sets[0].d_queue.get() == a.queue ? 0 : 1];
            HIP_TRY(ls.d_stream.reserve(size_t(s->n_cus) * size_t(pl.blocks_per_cu) * stream_scratch_bytes_per_block()));
            a.stream_scratch = ls.d_stream.get<uint32_t>();
        }
        // (grid, streams, events, max_blocks and the tile list are the AOT kernel's: only the function differs)
        const hipFunction_t jit = a.n_items ? scan_jit_function(s, a) : nullptr;
        pl.launch = [s, jit](const RenderArgs& ra, int nb, hipStream_t stream) {
            return jit ? launch_render_jit(s, jit, ra, nb, stream) : launch_render(ra, nb, stream);
        };
    }
    if ((rc = rpti::run_persistent(s, prm, a, d_out, st, pl))) return rc;
    if (!a.counters) return RPT_OK;
    HIP_TRY(hipStreamSynchronize(st));
    return f64 ? fetch_counters64(s, a) : rpti::fetch_counters(s, a);
}

int rpt_render_sample_device(rpt_scene* s, const rpt_camera* cam, const rpt_render_params* prm, uint32_t iterations,
                             uint64_t seed, uint32_t sample_offset, void* d_out_rgb, void* hip_stream) {
    if (!d_out_rgb) return fail(RPT_ERR_INVALID, "null output");
    return render_frame(s, cam, prm, iterations, seed, sample_offset, static_cast<double*>(d_out_rgb), static_cast<hipStream_t>(hip_stream));
}

int rpt_render_sample(rpt_scene* s, const rpt_camera* cam, const rpt_render_params* prm, uint32_t iterations,
                      uint64_t seed, uint32_t sample_offset, double* out_rgb) {
    if (!out_rgb) return fail(RPT_ERR_INVALID, "null output");
    if (int rc = render_frame(s, cam, prm, iterations, seed, sample_offset, nullptr, nullptr)) return rc;
    HIP_TRY(hipMemcpy(out_rgb, s->dev.d_out.get(), size_t(prm->width) * prm->height * 24, hipMemcpyDeviceToHost));
    // as ever: an fp32 render through this entry without counters leaves none behind (rpt_get_counters, rpt_scan_cull_counters: zeros)
    if (!s->opt.counters && !s->dev.arena64) return rpti::fetch_counters(s, RenderArgs{});
    return RPT_OK;
}
// What both entry points refuse before any device call.
static int check_sample_tiles(const rpt_scene* s, const rpt_camera* cam, const rpt_render_params* prm, uint32_t iterations, const void* tiles,
                              uint32_t n_tiles, const void* out) {
    if (!s || !cam || !prm) return fail(RPT_ERR_INVALID, "null argument");
    if (!out) return fail(RPT_ERR_INVALID, "null output");
    if (n_tiles && !tiles) return fail(RPT_ERR_INVALID, "null tile list");
    if (prm->width == 0 || prm->height == 0 || iterations == 0) return fail(RPT_ERR_INVALID, "empty render");
    if (uint64_t(prm->width) * prm->height > (1ull << 31)) return fail(RPT_ERR_INVALID, "image too large");
    if (prm->shard_count > 1) return fail(RPT_ERR_INVALID, "a tile-list render is not sharded: the list is the sharding");
    const uint64_t total = uint64_t((prm->width + 31) / 32) * ((prm->height + 31) / 32);
    if (n_tiles > total) return fail(RPT_ERR_INVALID, "more tiles listed than the frame has");
    return RPT_OK;
}
int rpt_render_sample_tiles_device(rpt_scene* s, const rpt_camera* cam, const rpt_render_params* prm, uint32_t iterations, uint64_t seed,
                                   uint32_t sample_offset, const void* d_tiles, uint32_t n_tiles, void* d_out_rgb, void* hip_stream) {
    if (int rc = check_sample_tiles(s, cam, prm, iterations, d_tiles, n_tiles, d_out_rgb)) return rc;
    if (!s->committed) return fail(RPT_ERR_STATE, "rpt_scene_commit must be called before rendering");
    if (n_tiles == 0) return RPT_OK;
    return render_frame(s, cam, prm, iterations, seed, sample_offset, static_cast<double*>(d_out_rgb), static_cast<hipStream_t>(hip_stream),
                        static_cast<const uint32_t*>(d_tiles), n_tiles);
}
int rpt_render_sample_tiles(rpt_scene* s, const rpt_camera* cam, const rpt_render_params* prm, uint32_t iterations, uint64_t seed,
                            uint32_t sample_offset, const uint32_t* tiles, uint32_t n_tiles, double* out_rgb) {
    if (int rc = check_sample_tiles(s, cam, prm, iterations, tiles, n_tiles, out_rgb)) return rc;
    {   // a host list is checked: ids in range and distinct
        const uint32_t total = ((prm->width + 31) / 32) * ((prm->height + 31) / 32);
        std::vector<bool> seen(total, false);
        for (uint32_t i = 0; i < n_tiles; i++) {
            if (tiles[i] >= total) return fail(RPT_ERR_INVALID, "tile id out of range");
            if (seen[tiles[i]]) return fail(RPT_ERR_INVALID, "tile id listed twice");
            seen[tiles[i]] = true;
        }
    }
    if (!s->committed) return fail(RPT_ERR_STATE, "rpt_scene_commit must be called before rendering");
    if (n_tiles == 0) return RPT_OK;
    HIP_TRY(hipSetDevice(s->device));
    const size_t bytes = size_t(prm->width) * prm->height * 24;
    double* d_out = rpti::scratch_out(s, bytes);
    if (!d_out) return fail(RPT_ERR_DEVICE, "out of device memory");
    rpti::DevMem d_list;   // this call's own upload, alive until the download below has synchronised
    HIP_TRY(d_list.reserve(size_t(n_tiles) * 4));
    HIP_TRY(hipMemcpy(d_list.get(), tiles, size_t(n_tiles) * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_out, out_rgb, bytes, hipMemcpyHostToDevice));   // the caller's values outside the listed tiles survive
    int rc = render_frame(s, cam, prm, iterations, seed, sample_offset, d_out, nullptr, d_list.get<uint32_t>(), n_tiles);
    const hipError_t e = hipMemcpy(out_rgb, d_out, bytes, hipMemcpyDeviceToHost);   // (also on failure: the list is freed after the stream is idle)
    if (rc) return rc;
    HIP_TRY(e);
    return RPT_OK;
}
// What rpt_render_features* refuse before any device call.
static int check_features(const rpt_scene* s, const rpt_camera* cam, const rpt_render_params* prm, uint32_t iterations, const void* albedo,
                          const void* normal, const void* depth) {
    if (!albedo && !normal && !depth) return fail(RPT_ERR_INVALID, "no feature plane requested");
    if (!s || !cam || !prm) return fail(RPT_ERR_INVALID, "null argument");
    if (prm->width == 0 || prm->height == 0 || iterations == 0) return fail(RPT_ERR_INVALID, "empty render");
    if (uint64_t(prm->width) * prm->height > (1ull << 31)) return fail(RPT_ERR_INVALID, "image too large");
    if (!s->committed) return fail(RPT_ERR_STATE, "rpt_scene_commit must be called before rendering");
    return RPT_OK;
}
// The feature pass on stream `st` into the requested device planes: records into the scene's own feature scratch (fp32 or
// reference-epsilon kernel, as the scene was committed), then the resolve.  A pass waits for the scene's previous one.
static int run_features(rpt_scene* s, const rpt_camera* cam, const rpt_render_params* prm, uint32_t iterations, uint64_t seed,
                        uint32_t sample_offset, double* d_albedo, double* d_normal, double* d_depth, hipStream_t st) {
    if (int rc = check_features(s, cam, prm, iterations, d_albedo, d_normal, d_depth)) return rc;
    RenderArgs a{};
    int rc = rpti::prepare_render(s, st, cam, prm, iterations, seed, sample_offset, a, 0, 0, 0, false);
    if (rc) return rc;
    const bool f64 = bool(s->dev.arena64);
    if (!launch_feature_resolve || (f64 ? !launch_features_f64 : !launch_features))
        return fail(RPT_ERR_UNSUPPORTED, "rpt_render_features: built without the kernels");
    if (s->dev.feat_used) HIP_TRY(hipStreamWaitEvent(st, s->dev.feat_done.get(), 0));
    else HIP_TRY(s->dev.feat_done.create(hipEventDisableTiming));
    s->dev.feat_used = true;
    const size_t slab_bytes = size_t(a.n_items) * 64;
    HIP_TRY(s->dev.d_feat_slab.reserve(std::max<size_t>(slab_bytes + size_t(a.n_owned) * 4, 16)));
    double* const slab = s->dev.d_feat_slab.get<double>();
    uint32_t* const ids = reinterpret_cast<uint32_t*>(s->dev.d_feat_slab.get<char>() + slab_bytes);
    const uint32_t shard_count = prm->shard_count == 0 ? 1 : prm->shard_count;
    if (shard_count > 1)   // the pixels of the other shards: 0 in every requested plane
        for (double* plane : {d_albedo, d_normal, d_depth})
            if (plane) HIP_TRY(hipMemsetAsync(plane, 0, size_t(prm->width) * prm->height * 24, st));
    if (f64) {
        rpt64::FeatureArgs64 q{};
        rpti::fill_args64(s, cam, prm, &a, q.a);
        q.slab = slab;
        q.ids = ids;
        HIP_TRY(launch_features_f64(q, st));
    } else {
        FeatureArgs q{};
        q.r = a;
        q.slab = slab;
        q.ids = ids;
        HIP_TRY(launch_features(q, st));
    }
    FeatureResolveArgs r{};
    r.tiles = a.tiles; r.tiles_x = a.tiles_x; r.n_owned = a.n_owned; r.n_chunks = a.n_chunks; r.n_items = a.n_items;
    r.width = a.width; r.height = a.height; r.iterations = a.iterations;
    r.slab = slab; r.ids = ids;
    r.albedo = d_albedo; r.normal = d_normal; r.depth = d_depth;
    HIP_TRY(launch_feature_resolve(r, st));
    HIP_TRY(hipEventRecord(s->dev.feat_done.get(), st));
    return RPT_OK;
}
int rpt_render_features_device(rpt_scene* s, const rpt_camera* cam, const rpt_render_params* prm, uint32_t iterations, uint64_t seed,
                               uint32_t sample_offset, void* d_albedo, void* d_normal, void* d_depth, void* hip_stream) {
    return run_features(s, cam, prm, iterations, seed, sample_offset, static_cast<double*>(d_albedo), static_cast<double*>(d_normal),
                        static_cast<double*>(d_depth), static_cast<hipStream_t>(hip_stream));
}
int rpt_render_features(rpt_scene* s, const rpt_camera* cam, const rpt_render_params* prm, uint32_t iterations, uint64_t seed,
                        uint32_t sample_offset, double* out_albedo, double* out_normal, double* out_depth) {
    if (int rc = check_features(s, cam, prm, iterations, out_albedo, out_normal, out_depth)) return rc;
    HIP_TRY(hipSetDevice(s->device));
    const size_t bytes = size_t(prm->width) * prm->height * 24;
    double* const outs[3] = {out_albedo, out_normal, out_depth};
    double* d[3] = {nullptr, nullptr, nullptr};
    size_t n_planes = 0;
    for (int k = 0; k < 3; k++) n_planes += outs[k] ? 1 : 0;
    // (the planes of the previous call have been copied out: its hipMemcpy waited for them)
    HIP_TRY(s->dev.d_feat_out.reserve(n_planes * bytes));
    for (int k = 0, i = 0; k < 3; k++)
        if (outs[k]) d[k] = s->dev.d_feat_out.get<double>() + size_t(i++) * (bytes / 8);
    int rc = run_features(s, cam, prm, iterations, seed, sample_offset, d[0], d[1], d[2], nullptr);
    if (rc) return rc;
    for (int k = 0; k < 3; k++)
        if (outs[k]) HIP_TRY(hipMemcpy(outs[k], d[k], bytes, hipMemcpyDeviceToHost));
    return RPT_OK;
}
int rpt_f64_mesh_tree_info(rpt_scene* s, uint64_t out[8]) {
    if (!s || !out) return fail(RPT_ERR_INVALID, "null argument");
    if (!s->committed) return fail(RPT_ERR_STATE, "rpt_scene_commit must be called first");
    if (!s->dev.arena64) return fail(RPT_ERR_STATE, "the scene was not committed with epsilon_policy = 1");
    for (int i = 0; i < 8; i++) out[i] = s->mesh_tree_info64[i];
    return RPT_OK;
}
int rpt_debug_epsilon_counters(rpt_scene* s, uint64_t out[12]) {
    if (!s || !out) return fail(RPT_ERR_INVALID, "null argument");
    if (!s->dev.arena64) return fail(RPT_ERR_STATE, "the scene was not committed with epsilon_policy = 1");
    for (int i = 0; i < 12; i++) out[i] = s->last_counters64[i];
    return RPT_OK;
}

// ---------------------------------------------------------------------------- Buffer on the device
rpt_buffer* rpt_buffer_create(int device, uint32_t width, uint32_t height, uint32_t filter_radius) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { fail(RPT_ERR_INVALID, "device index out of range"); return nullptr; }
    if (width == 0 || height == 0 || uint64_t(width) * height >= (1ull << 31)) { fail(RPT_ERR_INVALID, "bad buffer size"); return nullptr; }
    auto* b = new rpt_buffer();
    b->device = device;
    b->width = width;
    b->height = height;
    b->radius = filter_radius;
    const size_t n = size_t(width) * height;
    bool ok = hipSetDevice(device) == hipSuccess && b->d_sum.reserve(n * 24) == hipSuccess && b->d_sumsq.reserve(n * 8) == hipSuccess &&
              b->d_stage.reserve(n * 24) == hipSuccess && b->d_img.reserve(n * 3) == hipSuccess &&
              hipMemset(b->d_sum.get(), 0, n * 24) == hipSuccess && hipMemset(b->d_sumsq.get(), 0, n * 8) == hipSuccess;
    if (!ok) {
        fail(RPT_ERR_DEVICE, "rpt_buffer_create: device allocation failed");
        rpt_buffer_destroy(b);
        return nullptr;
    }
    return b;
}
void rpt_buffer_destroy(rpt_buffer* b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    delete b;
}
int rpt_buffer_add_samples_device(rpt_buffer* b, const void* d_rgb, void* hip_stream) {
    if (!b || !d_rgb) return fail(RPT_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(launch_buffer_add(b->width * b->height, static_cast<const double*>(d_rgb), b->d_sum.get<double>(), b->d_sumsq.get<double>(),
                              static_cast<hipStream_t>(hip_stream)));
    b->n_batches++;
    return RPT_OK;
}
int rpt_buffer_add_samples(rpt_buffer* b, const double* rgb) {
    if (!b || !rgb) return fail(RPT_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipMemcpy(b->d_stage.get(), rgb, size_t(b->width) * b->height * 24, hipMemcpyHostToDevice));
    return rpt_buffer_add_samples_device(b, b->d_stage.get(), nullptr);
}
int rpt_buffer_image(rpt_buffer* b, uint8_t* out_rgb8) {
    if (!b || !out_rgb8) return fail(RPT_ERR_INVALID, "null argument");
    if (b->n_batches == 0) return fail(RPT_ERR_STATE, "Pixel found with no samples");  // the reference's assert (buffer.rs:89)
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipDeviceSynchronize());  // batches may have been added on other streams
    if (b->d_extra) {   // tiles with different batch counts: the window's sums over the window's sample count (buffer.rs:75-93)
        if (!launch_buffer_image_tiles) return fail(RPT_ERR_UNSUPPORTED, "rpt_buffer_image: built without the kernels");
        HIP_TRY(launch_buffer_image_tiles(b->view(), b->radius, b->d_sum.get<double>(), b->d_img.get<uint8_t>(), nullptr));
    } else
        HIP_TRY(launch_buffer_image(b->width, b->height, b->radius, b->n_batches, b->d_sum.get<double>(), b->d_img.get<uint8_t>(), nullptr));
    HIP_TRY(hipMemcpy(out_rgb8, b->d_img.get(), size_t(b->width) * b->height * 3, hipMemcpyDeviceToHost));
    return RPT_OK;
}
int rpt_buffer_variance(rpt_buffer* b, double* out) {
    if (!b || !out) return fail(RPT_ERR_INVALID, "null argument");
    if (b->n_batches < 2) { *out = std::numeric_limits<double>::quiet_NaN(); return RPT_OK; }  // 0/0 in the reference too
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipDeviceSynchronize());
    const size_t n = size_t(b->width) * b->height;
    if (b->d_extra) {
        if (!launch_buffer_variance_tiles) return fail(RPT_ERR_UNSUPPORTED, "rpt_buffer_variance: built without the kernels");
        HIP_TRY(launch_buffer_variance_tiles(b->view(), b->d_sum.get<double>(), b->d_sumsq.get<double>(), b->d_stage.get<double>(), nullptr));
    } else
        HIP_TRY(launch_buffer_variance(uint32_t(n), b->n_batches, b->d_sum.get<double>(), b->d_sumsq.get<double>(), b->d_stage.get<double>(), nullptr));
    std::vector<double> v(n);
    HIP_TRY(hipMemcpy(v.data(), b->d_stage.get(), n * 8, hipMemcpyDeviceToHost));
    double acc = 0.0;
    for (double x : v) acc += x;  // pixel order, as buffer.rs:63-72
    *out = acc / double(n);
    return RPT_OK;
}
int rpt_buffer_batches(rpt_buffer* b, uint32_t* n) {
    if (!b || !n) return fail(RPT_ERR_INVALID, "null argument");
    *n = b->n_batches;
    return RPT_OK;
}
// Renderer::sample(&self, iterations, &mut Buffer), src/renderer.rs:158-171: the frame never leaves the device.
int rpt_render_into_buffer(rpt_scene* s, const rpt_camera* cam, const rpt_render_params* prm, uint32_t iterations,
                           uint64_t seed, uint32_t sample_offset, rpt_buffer* b) {
    if (!b) return fail(RPT_ERR_INVALID, "null buffer");
    if (!s || !prm) return fail(RPT_ERR_INVALID, "null argument");
    if (prm->width != b->width || prm->height != b->height) return fail(RPT_ERR_INVALID, "Invalid sample dimension");  // buffer.rs:33-36
    if (s->committed && s->device != b->device) return fail(RPT_ERR_INVALID, "buffer and scene live on different devices");
    if (int rc = render_frame(s, cam, prm, iterations, seed, sample_offset, b->d_stage.get<double>(), nullptr)) return rc;
    return rpt_buffer_add_samples_device(b, b->d_stage.get(), nullptr);
}

// ---------------------------------------------------------------------------- adaptive sampling by tile (adaptive.hip)
int rpt_buffer_add_samples_tiles_device(rpt_buffer* b, const void* d_rgb, const void* d_tiles, uint32_t n_tiles, void* hip_stream) {
    if (!b || !d_rgb || (n_tiles && !d_tiles)) return fail(RPT_ERR_INVALID, "null argument");
    if (n_tiles > b->n_tiles()) return fail(RPT_ERR_INVALID, "more tiles listed than the frame has");
    if (n_tiles == 0) return RPT_OK;
    if (!launch_buffer_add_tiles) return fail(RPT_ERR_UNSUPPORTED, "rpt_buffer_add_samples_tiles_device: built without the kernels");
    HIP_TRY(hipSetDevice(b->device));
    const hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (!b->d_extra) {
        HIP_TRY(b->d_extra.reserve(size_t(b->n_tiles()) * 4));
        HIP_TRY(hipMemsetAsync(b->d_extra.get(), 0, size_t(b->n_tiles()) * 4, st));
    }
    HIP_TRY(launch_buffer_add_tiles(b->view(), static_cast<const double*>(d_rgb), b->d_sum.get<double>(), b->d_sumsq.get<double>(),
                                    b->d_extra.get<uint32_t>(), static_cast<const uint32_t*>(d_tiles), n_tiles, st));
    return RPT_OK;
}
int rpt_buffer_tile_batches(rpt_buffer* b, uint32_t* out, uint64_t capacity) {
    if (!b || !out) return fail(RPT_ERR_INVALID, "null argument");
    if (capacity < b->n_tiles()) return fail(RPT_ERR_INVALID, "rpt_buffer_tile_batches: capacity below tiles_x * tiles_y");
    std::fill(out, out + b->n_tiles(), 0u);
    if (b->d_extra) {
        HIP_TRY(hipSetDevice(b->device));
        HIP_TRY(hipDeviceSynchronize());  // batches may have been added on other streams
        HIP_TRY(hipMemcpy(out, b->d_extra.get(), size_t(b->n_tiles()) * 4, hipMemcpyDeviceToHost));
    }
    for (uint32_t t = 0; t < b->n_tiles(); t++) out[t] += b->n_batches;
    return RPT_OK;
}
// What rpt_buffer_refine_tiles and rpt_render_adaptive refuse in their parameters, before any device call.
static int check_adaptive(const rpt_adaptive_params* p) {
    if (!p) return fail(RPT_ERR_INVALID, "null adaptive parameters");
    if (p->spp_per_batch == 0) return fail(RPT_ERR_INVALID, "spp_per_batch must be at least 1");
    if (p->min_batches < 2) return fail(RPT_ERR_INVALID, "min_batches must be at least 2: a tile's error needs a variance");
    if (p->max_batches < p->min_batches) return fail(RPT_ERR_INVALID, "max_batches must be at least min_batches");
    if (uint64_t(p->max_batches) * p->spp_per_batch > 0xFFFFFFFFull) return fail(RPT_ERR_INVALID, "max_batches * spp_per_batch must fit 32 bits");
    if (!(p->threshold >= 0.0)) return fail(RPT_ERR_INVALID, "threshold must be >= 0 (+inf allowed)");
    if (!(p->floor > 0.0) || std::isinf(p->floor)) return fail(RPT_ERR_INVALID, "floor must be finite and > 0");
    return RPT_OK;
}
static int run_tile_errors(rpt_buffer* b, double floor, double* d_err, hipStream_t st) {
    if (b->n_batches < 2) return fail(RPT_ERR_STATE, "a tile's error needs at least 2 full-frame batches");
    if (!launch_tile_errors || !launch_tile_select) return fail(RPT_ERR_UNSUPPORTED, "adaptive sampling: built without the kernels");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(launch_tile_errors(b->view(), floor, b->d_sum.get<double>(), b->d_sumsq.get<double>(), d_err, st));
    return RPT_OK;
}
int rpt_buffer_tile_errors_device(rpt_buffer* b, double floor, void* d_err, void* hip_stream) {
    if (!(floor > 0.0) || std::isinf(floor)) return fail(RPT_ERR_INVALID, "floor must be finite and > 0");
    if (!b || !d_err) return fail(RPT_ERR_INVALID, "null argument");
    return run_tile_errors(b, floor, static_cast<double*>(d_err), static_cast<hipStream_t>(hip_stream));
}
int rpt_buffer_refine_tiles(rpt_buffer* b, const rpt_adaptive_params* p, void* d_tiles_out, uint32_t* n_out, void* d_err, void* hip_stream) {
    if (int rc = check_adaptive(p)) return rc;
    if (!b || !d_tiles_out || !n_out) return fail(RPT_ERR_INVALID, "null argument");
    if (b->n_batches < 2) return fail(RPT_ERR_STATE, "a tile's error needs at least 2 full-frame batches");
    HIP_TRY(hipSetDevice(b->device));
    const hipStream_t st = static_cast<hipStream_t>(hip_stream);
    // the errors when the caller keeps none, and the count behind them
    HIP_TRY(b->d_tile_err.reserve(size_t(b->n_tiles()) * 8 + 8));
    double* const err = d_err ? static_cast<double*>(d_err) : b->d_tile_err.get<double>();
    uint32_t* const d_count = reinterpret_cast<uint32_t*>(b->d_tile_err.get<double>() + b->n_tiles());
    if (int rc = run_tile_errors(b, p->floor, err, st)) return rc;
    HIP_TRY(launch_tile_select(b->view(), p->threshold * p->threshold, p->max_batches, err, static_cast<uint32_t*>(d_tiles_out), d_count, st));
    HIP_TRY(hipStreamSynchronize(st));   // the one synchronisation and the one read-back of a round, 4 bytes
    HIP_TRY(hipMemcpy(n_out, d_count, 4, hipMemcpyDeviceToHost));
    return RPT_OK;
}
int rpt_render_adaptive(rpt_scene* s, const rpt_camera* cam, const rpt_render_params* prm, const rpt_adaptive_params* p, uint64_t seed,
                        rpt_buffer* b, uint64_t stats[4]) {
    if (!s || !cam || !prm) return fail(RPT_ERR_INVALID, "null argument");
    if (int rc = check_adaptive(p)) return rc;
    if (prm->shard_count > 1) return fail(RPT_ERR_INVALID, "an adaptive render is not sharded");
    if (!b) return fail(RPT_ERR_INVALID, "null buffer");
    if (prm->width != b->width || prm->height != b->height) return fail(RPT_ERR_INVALID, "Invalid sample dimension");  // buffer.rs:33-36
    if (s->committed && s->device != b->device) return fail(RPT_ERR_INVALID, "buffer and scene live on different devices");
    if (b->n_batches || b->d_extra) return fail(RPT_ERR_STATE, "rpt_render_adaptive needs an empty buffer");
    for (uint32_t k = 0; k < p->min_batches; k++)
        if (int rc = rpt_render_into_buffer(s, cam, prm, p->spp_per_batch, seed, k * p->spp_per_batch, b)) return rc;
    HIP_TRY(b->d_active.reserve(size_t(b->n_tiles()) * 4));
    uint32_t* const d_active = b->d_active.get<uint32_t>();
    uint64_t rounds = 0, tile_batches = uint64_t(p->min_batches) * b->n_tiles();
    // A tile's error does not change while it is not sampled: the active set only shrinks, and every active tile holds k batches.
    for (uint32_t k = p->min_batches; k < p->max_batches; k++) {
        uint32_t n_active = 0;
        if (int rc = rpt_buffer_refine_tiles(b, p, d_active, &n_active, nullptr, nullptr)) return rc;
        if (n_active == 0) break;
        if (int rc = rpt_render_sample_tiles_device(s, cam, prm, p->spp_per_batch, seed, k * p->spp_per_batch, d_active, n_active, b->d_stage.get(), nullptr))
            return rc;
        if (int rc = rpt_buffer_add_samples_tiles_device(b, b->d_stage.get(), d_active, n_active, nullptr)) return rc;
        rounds++;
        tile_batches += n_active;
    }
    if (stats) {
        std::vector<uint32_t> n(b->n_tiles());
        if (int rc = rpt_buffer_tile_batches(b, n.data(), n.size())) return rc;
        stats[0] = rounds;
        stats[1] = tile_batches;
        stats[2] = uint64_t(std::count(n.begin(), n.end(), p->max_batches));
        stats[3] = b->n_tiles();
    }
    return RPT_OK;
}

// ---------------------------------------------------------------------------- denoiser on the device (denoise.hip)
// The largest step whose passes stage their tile in LDS when "denoise_stage" is -1: both staged steps, each faster than the gather by
// 0.08 ms of 0.16 at 1024 x 1024, twenty times the run-to-run spread ("Denoiser").
static constexpr int64_t kDenoiseStageDefault = 2;
struct rpt_denoiser {
    int device = 0;
    uint32_t width = 0, height = 0;
    int64_t stage = 0;                 // passes of step <= stage use the staged form
    rpti::DevMem d_rec[2], d_ids;      // ping-pong records (8 doubles per pixel) and the ids
    rpti::DevMem d_host;               // rpt_denoise: the planes of the host entry point
    rpti::DevMem d_frame;              // rpt_buffer_denoised_image: mean, variance, filtered frame
    rpti::Event done;                  // recorded after the last kernel of a call: the next call waits for it, whatever its stream
    bool used = false;
};
rpt_denoiser* rpt_denoiser_create(int device, uint32_t width, uint32_t height) {
    if (width == 0 || height == 0 || uint64_t(width) * height >= (1ull << 31)) { fail(RPT_ERR_INVALID, "bad denoiser size"); return nullptr; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { fail(RPT_ERR_INVALID, "device index out of range"); return nullptr; }
    auto* d = new rpt_denoiser();
    d->device = device;
    d->width = width;
    d->height = height;
    {
        std::lock_guard<std::mutex> lock(g_defaults_mutex);
        d->stage = g_defaults.denoise_stage < 0 ? kDenoiseStageDefault : g_defaults.denoise_stage;
    }
    const size_t n = size_t(width) * height;
    const bool ok = hipSetDevice(device) == hipSuccess && d->d_rec[0].reserve(n * 64) == hipSuccess && d->d_rec[1].reserve(n * 64) == hipSuccess &&
                    d->d_ids.reserve(n * 8) == hipSuccess && d->done.create(hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        fail(RPT_ERR_DEVICE, "rpt_denoiser_create: device allocation failed");
        rpt_denoiser_destroy(d);
        return nullptr;
    }
    return d;
}
void rpt_denoiser_destroy(rpt_denoiser* d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    delete d;
}
// What rpt_denoise* refuse before any device call.
static int check_denoise(const rpt_denoiser* d, const rpt_denoise_params* prm, const void* rgb, const void* var, const void* albedo,
                         const void* normal, const void* depth, const void* out, const void* out_var) {
    if (!prm) return fail(RPT_ERR_INVALID, "null denoise parameters");
    if (prm->passes < 1 || prm->passes > 8) return fail(RPT_ERR_INVALID, "passes must be 1..8");
    if (prm->flags & ~(RPT_DENOISE_DEMODULATE | RPT_DENOISE_MATCH_ID)) return fail(RPT_ERR_INVALID, "unknown denoise flag");
    for (double sg : {prm->sigma_color, prm->sigma_normal, prm->sigma_depth})
        if (!(sg >= 0.0) || std::isinf(sg)) return fail(RPT_ERR_INVALID, "a sigma must be finite and >= 0 (0: the term is off)");
    if (!rgb || !out) return fail(RPT_ERR_INVALID, "null frame");
    if (prm->sigma_color > 0.0 && !var) return fail(RPT_ERR_INVALID, "sigma_color > 0 needs the variance plane");
    if (prm->sigma_normal > 0.0 && !normal) return fail(RPT_ERR_INVALID, "sigma_normal > 0 needs the normal plane");
    if (prm->sigma_depth > 0.0 && !depth) return fail(RPT_ERR_INVALID, "sigma_depth > 0 needs the depth plane");
    if ((prm->flags & RPT_DENOISE_DEMODULATE) && !albedo) return fail(RPT_ERR_INVALID, "RPT_DENOISE_DEMODULATE needs the albedo plane");
    if ((prm->flags & RPT_DENOISE_MATCH_ID) && !depth) return fail(RPT_ERR_INVALID, "RPT_DENOISE_MATCH_ID needs the depth plane");
    for (const void* o : {out, out_var})
        for (const void* in : {rgb, var, albedo, normal, depth})
            if (o && o == in) return fail(RPT_ERR_INVALID, "an output must not be one of the inputs");
    if (out == out_var) return fail(RPT_ERR_INVALID, "out and out_var must differ");
    if (!d) return fail(RPT_ERR_INVALID, "null denoiser");
    return RPT_OK;
}
static int run_denoise(rpt_denoiser* d, const rpt_denoise_params* prm, const double* d_rgb, const double* d_var, const double* d_albedo,
                       const double* d_normal, const double* d_depth, double* d_out, double* d_out_var, hipStream_t st) {
    if (int rc = check_denoise(d, prm, d_rgb, d_var, d_albedo, d_normal, d_depth, d_out, d_out_var)) return rc;
    if (!launch_denoise_prepare || !launch_denoise_pass) return fail(RPT_ERR_UNSUPPORTED, "rpt_denoise: built without the kernels");
    HIP_TRY(hipSetDevice(d->device));
    if (d->used) HIP_TRY(hipStreamWaitEvent(st, d->done.get(), 0));
    d->used = true;
    DenoisePrepareArgs q{};
    q.n_pixels = d->width * d->height;
    q.flags = prm->flags;
    q.rgb = d_rgb; q.var = d_var; q.albedo = d_albedo; q.normal = d_normal; q.depth = d_depth;
    q.rec = d->d_rec[0].get<double>();
    q.ids = d->d_ids.get<double>();
    HIP_TRY(launch_denoise_prepare(q, st));
    for (uint32_t i = 0; i < prm->passes; i++) {
        DenoisePassArgs a{};
        a.width = d->width; a.height = d->height; a.step = 1u << i; a.flags = prm->flags;
        a.terms = (prm->sigma_color > 0.0 ? 1u : 0u) | (prm->sigma_normal > 0.0 ? 2u : 0u) | (prm->sigma_depth > 0.0 ? 4u : 0u);
        a.sigma_color2 = prm->sigma_color * prm->sigma_color;
        a.a_n = 1.0 / prm->sigma_normal;
        a.a_z = 1.0 / (prm->sigma_depth * double(a.step));
        a.rec_in = d->d_rec[i & 1].get<double>();
        a.ids = d->d_ids.get<double>();
        a.albedo = d_albedo;
        if (i + 1 == prm->passes) { a.out = d_out; a.out_var = d_out_var; }
        else a.rec_out = d->d_rec[(i + 1) & 1].get<double>();
        HIP_TRY(launch_denoise_pass(a, int64_t(a.step) <= d->stage, st));
    }
    HIP_TRY(hipEventRecord(d->done.get(), st));
    return RPT_OK;
}
int rpt_denoise_device(rpt_denoiser* d, const rpt_denoise_params* prm, const void* d_rgb, const void* d_var, const void* d_albedo,
                       const void* d_normal, const void* d_depth, void* d_out, void* d_out_var, void* hip_stream) {
    return run_denoise(d, prm, static_cast<const double*>(d_rgb), static_cast<const double*>(d_var), static_cast<const double*>(d_albedo),
                       static_cast<const double*>(d_normal), static_cast<const double*>(d_depth), static_cast<double*>(d_out),
                       static_cast<double*>(d_out_var), static_cast<hipStream_t>(hip_stream));
}
int rpt_denoise(rpt_denoiser* d, const rpt_denoise_params* prm, const double* rgb, const double* var, const double* albedo,
                const double* normal, const double* depth, double* out, double* out_var) {
    if (int rc = check_denoise(d, prm, rgb, var, albedo, normal, depth, out, out_var)) return rc;
    HIP_TRY(hipSetDevice(d->device));
    const size_t n = size_t(d->width) * d->height;
    // rgb, albedo, normal, depth, out: 3 n each; var, out_var: n each
    HIP_TRY(d->d_host.reserve(17 * n * 8));
    double* const base = d->d_host.get<double>();
    const double* const ins[5] = {rgb, albedo, normal, depth, var};
    double* dev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    for (int k = 0; k < 5; k++)
        if (ins[k]) {
            dev[k] = base + size_t(k) * 3 * n;
            HIP_TRY(hipMemcpy(dev[k], ins[k], (k == 4 ? n : 3 * n) * 8, hipMemcpyHostToDevice));
        }
    double* const d_out = base + 13 * n;
    double* const d_out_var = out_var ? base + 16 * n : nullptr;
    if (int rc = run_denoise(d, prm, dev[0], dev[4], dev[1], dev[2], dev[3], d_out, d_out_var, nullptr)) return rc;
    HIP_TRY(hipMemcpy(out, d_out, 3 * n * 8, hipMemcpyDeviceToHost));
    if (out_var) HIP_TRY(hipMemcpy(out_var, d_out_var, n * 8, hipMemcpyDeviceToHost));
    return RPT_OK;
}
int rpt_buffer_mean_device(rpt_buffer* b, void* d_rgb, void* d_var, void* hip_stream) {
    if (!b || !d_rgb) return fail(RPT_ERR_INVALID, "null argument");
    if (d_rgb == d_var) return fail(RPT_ERR_INVALID, "d_rgb and d_var must differ");
    if (b->n_batches < 2) return fail(RPT_ERR_STATE, "the variance of the mean needs at least 2 batches");
    if (!launch_buffer_mean) return fail(RPT_ERR_UNSUPPORTED, "rpt_buffer_mean_device: built without the kernels");
    HIP_TRY(hipSetDevice(b->device));
    if (b->d_extra) {
        if (!launch_buffer_mean_tiles) return fail(RPT_ERR_UNSUPPORTED, "rpt_buffer_mean_device: built without the kernels");
        HIP_TRY(launch_buffer_mean_tiles(b->view(), b->d_sum.get<double>(), b->d_sumsq.get<double>(), static_cast<double*>(d_rgb),
                                         static_cast<double*>(d_var), static_cast<hipStream_t>(hip_stream)));
        return RPT_OK;
    }
    HIP_TRY(launch_buffer_mean(b->width * b->height, b->n_batches, b->d_sum.get<double>(), b->d_sumsq.get<double>(), static_cast<double*>(d_rgb),
                               static_cast<double*>(d_var), static_cast<hipStream_t>(hip_stream)));
    return RPT_OK;
}
int rpt_buffer_denoised_image(rpt_buffer* b, rpt_denoiser* d, const rpt_denoise_params* prm, const void* d_albedo, const void* d_normal,
                              const void* d_depth, uint8_t* out_rgb8) {
    if (!b || !d || !out_rgb8) return fail(RPT_ERR_INVALID, "null argument");
    if (b->device != d->device) return fail(RPT_ERR_INVALID, "buffer and denoiser live on different devices");
    if (b->width != d->width || b->height != d->height) return fail(RPT_ERR_INVALID, "buffer and denoiser have different sizes");
    // (the frame and its variance come from the buffer: placeholders that are no plane of the caller's)
    if (int rc = check_denoise(d, prm, b, prm && prm->sigma_color > 0.0 ? d : nullptr, d_albedo, d_normal, d_depth, out_rgb8, nullptr)) return rc;
    if (b->n_batches < 2) return fail(RPT_ERR_STATE, "the variance of the mean needs at least 2 batches");
    if (!launch_buffer_mean || !launch_color_bytes) return fail(RPT_ERR_UNSUPPORTED, "rpt_buffer_denoised_image: built without the kernels");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipDeviceSynchronize());  // batches and planes may have been written on other streams
    const size_t n = size_t(b->width) * b->height;
    HIP_TRY(d->d_frame.reserve(7 * n * 8));
    double* const mean = d->d_frame.get<double>();
    double* const var = mean + 3 * n;
    double* const out = mean + 4 * n;
    if (int rc = rpt_buffer_mean_device(b, mean, var, nullptr)) return rc;
    if (int rc = run_denoise(d, prm, mean, var, static_cast<const double*>(d_albedo), static_cast<const double*>(d_normal),
                             static_cast<const double*>(d_depth), out, nullptr, nullptr))
        return rc;
    HIP_TRY(launch_color_bytes(3 * n, out, b->d_img.get<uint8_t>(), nullptr));
    HIP_TRY(hipMemcpy(out_rgb8, b->d_img.get(), n * 3, hipMemcpyDeviceToHost));
    return RPT_OK;
}

// ---------------------------------------------------------------------------- guided upsampling (upsample.hip)
// What rpt_upsample* refuse before any device call, in the order include/rpt_hip.h states.
static int check_upsample(const rpt_upsample_params* prm, uint32_t w, uint32_t h, const void* lo_rgb, const void* lo_var, const void* lo_albedo,
                          const void* lo_normal, const void* lo_depth, const void* hi_albedo, const void* hi_normal, const void* hi_depth,
                          const void* out, const void* out_var) {
    if (!prm) return fail(RPT_ERR_INVALID, "null upsample parameters");
    if (prm->scale < 2 || prm->scale > 4) return fail(RPT_ERR_INVALID, "scale must be 2, 3 or 4");
    if (prm->radius < 1 || prm->radius > 2) return fail(RPT_ERR_INVALID, "radius must be 1 or 2");
    if (prm->flags & ~(RPT_UPSAMPLE_DEMODULATE | RPT_UPSAMPLE_MATCH_ID)) return fail(RPT_ERR_INVALID, "unknown upsample flag");
    for (double sg : {prm->sigma_normal, prm->sigma_depth})
        if (!(sg >= 0.0) || std::isinf(sg)) return fail(RPT_ERR_INVALID, "a sigma must be finite and >= 0 (0: the term is off)");
    if (w == 0 || h == 0) return fail(RPT_ERR_INVALID, "empty low-resolution frame");
    const uint64_t W = uint64_t(w) * prm->scale, H = uint64_t(h) * prm->scale;
    if (W >= (1ull << 32) || H >= (1ull << 32) || W * H >= (1ull << 31)) return fail(RPT_ERR_INVALID, "the full-resolution frame is too large");
    if (!lo_rgb || !out) return fail(RPT_ERR_INVALID, "null frame");
    if (prm->sigma_normal > 0.0 && !lo_normal) return fail(RPT_ERR_INVALID, "sigma_normal > 0 needs the low-resolution normal plane");
    if (prm->sigma_normal > 0.0 && !hi_normal) return fail(RPT_ERR_INVALID, "sigma_normal > 0 needs the full-resolution normal plane");
    if (prm->sigma_depth > 0.0 && !lo_depth) return fail(RPT_ERR_INVALID, "sigma_depth > 0 needs the low-resolution depth plane");
    if (prm->sigma_depth > 0.0 && !hi_depth) return fail(RPT_ERR_INVALID, "sigma_depth > 0 needs the full-resolution depth plane");
    if ((prm->flags & RPT_UPSAMPLE_DEMODULATE) && !lo_albedo) return fail(RPT_ERR_INVALID, "RPT_UPSAMPLE_DEMODULATE needs the low-resolution albedo plane");
    if ((prm->flags & RPT_UPSAMPLE_DEMODULATE) && !hi_albedo) return fail(RPT_ERR_INVALID, "RPT_UPSAMPLE_DEMODULATE needs the full-resolution albedo plane");
    if ((prm->flags & RPT_UPSAMPLE_MATCH_ID) && !lo_depth) return fail(RPT_ERR_INVALID, "RPT_UPSAMPLE_MATCH_ID needs the low-resolution depth plane");
    if ((prm->flags & RPT_UPSAMPLE_MATCH_ID) && !hi_depth) return fail(RPT_ERR_INVALID, "RPT_UPSAMPLE_MATCH_ID needs the full-resolution depth plane");
    for (const void* o : {out, out_var})
        for (const void* in : {lo_rgb, lo_var, lo_albedo, lo_normal, lo_depth, hi_albedo, hi_normal, hi_depth})
            if (o && o == in) return fail(RPT_ERR_INVALID, "an output must not be one of the inputs");
    if (out == out_var) return fail(RPT_ERR_INVALID, "out_rgb and out_var must differ");
    return RPT_OK;
}
// The launch of a checked call: the planes a term or flag that is off would read are not handed on.
static int run_upsample(const rpt_upsample_params* prm, uint32_t w, uint32_t h, const void* lo_rgb, const void* lo_var, const void* lo_albedo,
                        const void* lo_normal, const void* lo_depth, const void* hi_albedo, const void* hi_normal, const void* hi_depth, void* out,
                        void* out_var, hipStream_t st) {
    if (!launch_upsample) return fail(RPT_ERR_UNSUPPORTED, "rpt_upsample: built without the kernels");
    UpsampleArgs a{};
    a.width = w; a.height = h; a.scale = prm->scale; a.radius = prm->radius; a.flags = prm->flags;
    a.terms = (prm->sigma_normal > 0.0 ? 1u : 0u) | (prm->sigma_depth > 0.0 ? 2u : 0u);
    a.a_n = 1.0 / prm->sigma_normal;
    a.a_z = 1.0 / (prm->sigma_depth * double(prm->scale));
    const bool demod = prm->flags & RPT_UPSAMPLE_DEMODULATE, depth = (a.terms & 2u) || (prm->flags & RPT_UPSAMPLE_MATCH_ID);
    a.lo_rgb = static_cast<const double*>(lo_rgb);
    a.lo_var = static_cast<const double*>(lo_var);
    a.lo_albedo = demod ? static_cast<const double*>(lo_albedo) : nullptr;
    a.hi_albedo = demod ? static_cast<const double*>(hi_albedo) : nullptr;
    a.lo_normal = (a.terms & 1u) ? static_cast<const double*>(lo_normal) : nullptr;
    a.hi_normal = (a.terms & 1u) ? static_cast<const double*>(hi_normal) : nullptr;
    a.lo_depth = depth ? static_cast<const double*>(lo_depth) : nullptr;
    a.hi_depth = depth ? static_cast<const double*>(hi_depth) : nullptr;
    a.out_rgb = static_cast<double*>(out);
    a.out_var = static_cast<double*>(out_var);
    HIP_TRY(launch_upsample(a, st));
    return RPT_OK;
}
int rpt_upsample_device(const rpt_upsample_params* prm, uint32_t lo_width, uint32_t lo_height, const void* d_lo_rgb, const void* d_lo_var,
                        const void* d_lo_albedo, const void* d_lo_normal, const void* d_lo_depth, const void* d_hi_albedo,
                        const void* d_hi_normal, const void* d_hi_depth, void* d_out_rgb, void* d_out_var, void* hip_stream) {
    if (int rc = check_upsample(prm, lo_width, lo_height, d_lo_rgb, d_lo_var, d_lo_albedo, d_lo_normal, d_lo_depth, d_hi_albedo, d_hi_normal,
                                d_hi_depth, d_out_rgb, d_out_var))
        return rc;
    return run_upsample(prm, lo_width, lo_height, d_lo_rgb, d_lo_var, d_lo_albedo, d_lo_normal, d_lo_depth, d_hi_albedo, d_hi_normal, d_hi_depth,
                        d_out_rgb, d_out_var, static_cast<hipStream_t>(hip_stream));
}
int rpt_upsample(int device, const rpt_upsample_params* prm, uint32_t lo_width, uint32_t lo_height, const double* lo_rgb, const double* lo_var,
                 const double* lo_albedo, const double* lo_normal, const double* lo_depth, const double* hi_albedo, const double* hi_normal,
                 const double* hi_depth, double* out_rgb, double* out_var) {
    if (int rc = check_upsample(prm, lo_width, lo_height, lo_rgb, lo_var, lo_albedo, lo_normal, lo_depth, hi_albedo, hi_normal, hi_depth, out_rgb,
                                out_var))
        return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(RPT_ERR_INVALID, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    const size_t n = size_t(lo_width) * lo_height, N = n * prm->scale * prm->scale;
    // low resolution: rgb, albedo, normal, depth 3 n each, var n; full resolution: albedo, normal, depth, out 3 N each, out_var N
    rpti::DevMem mem;
    HIP_TRY(mem.reserve((13 * n + 13 * N) * 8));
    double* const base = mem.get<double>();
    const double* const ins[8] = {lo_rgb, lo_albedo, lo_normal, lo_depth, lo_var, hi_albedo, hi_normal, hi_depth};
    const size_t at[8] = {0, 3 * n, 6 * n, 9 * n, 12 * n, 13 * n, 13 * n + 3 * N, 13 * n + 6 * N};
    const size_t len[8] = {3 * n, 3 * n, 3 * n, 3 * n, n, 3 * N, 3 * N, 3 * N};
    double* dev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    for (int k = 0; k < 8; k++)
        if (ins[k]) {
            dev[k] = base + at[k];
            HIP_TRY(hipMemcpy(dev[k], ins[k], len[k] * 8, hipMemcpyHostToDevice));
        }
    double* const d_out = base + 13 * n + 9 * N;
    double* const d_out_var = out_var ? base + 13 * n + 12 * N : nullptr;
    if (int rc = run_upsample(prm, lo_width, lo_height, dev[0], dev[4], dev[1], dev[2], dev[3], dev[5], dev[6], dev[7], d_out, d_out_var, nullptr))
        return rc;
    HIP_TRY(hipMemcpy(out_rgb, d_out, 3 * N * 8, hipMemcpyDeviceToHost));
    if (out_var) HIP_TRY(hipMemcpy(out_var, d_out_var, N * 8, hipMemcpyDeviceToHost));
    return RPT_OK;
}
int rpt_image_bytes_device(const void* d_rgb, uint32_t width, uint32_t height, uint8_t* out_rgb8_host, void* hip_stream) {
    if (!d_rgb || !out_rgb8_host) return fail(RPT_ERR_INVALID, "null argument");
    if (width == 0 || height == 0 || uint64_t(width) * height >= (1ull << 31)) return fail(RPT_ERR_INVALID, "bad image size");
    if (!launch_color_bytes) return fail(RPT_ERR_UNSUPPORTED, "rpt_image_bytes_device: built without the kernels");
    const size_t n = size_t(width) * height;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    rpti::DevMem img;
    HIP_TRY(img.reserve(3 * n));
    HIP_TRY(launch_color_bytes(3 * n, static_cast<const double*>(d_rgb), img.get<uint8_t>(), st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpy(out_rgb8_host, img.get(), 3 * n, hipMemcpyDeviceToHost));
    return RPT_OK;
}
int rpt_buffer_upsampled_image(rpt_buffer* b, rpt_denoiser* d, const rpt_denoise_params* dprm, const rpt_upsample_params* prm,
                               const void* d_lo_albedo, const void* d_lo_normal, const void* d_lo_depth, const void* d_hi_albedo,
                               const void* d_hi_normal, const void* d_hi_depth, uint8_t* out_rgb8) {
    if (!b || !out_rgb8) return fail(RPT_ERR_INVALID, "null argument");
    // (the frame and its variance come from the buffer: placeholders that are no plane of the caller's)
    if (int rc = check_upsample(prm, b->width, b->height, b, nullptr, d_lo_albedo, d_lo_normal, d_lo_depth, d_hi_albedo, d_hi_normal, d_hi_depth,
                                out_rgb8, nullptr))
        return rc;
    if (d) {
        if (int rc = check_denoise(d, dprm, b, dprm && dprm->sigma_color > 0.0 ? d : nullptr, d_lo_albedo, d_lo_normal, d_lo_depth, out_rgb8, nullptr))
            return rc;
        if (b->device != d->device) return fail(RPT_ERR_INVALID, "buffer and denoiser live on different devices");
        if (b->width != d->width || b->height != d->height) return fail(RPT_ERR_INVALID, "buffer and denoiser have different sizes");
    }
    if (b->n_batches < 2) return fail(RPT_ERR_STATE, "the variance of the mean needs at least 2 batches");
    if (!launch_buffer_mean || !launch_color_bytes || !launch_upsample)
        return fail(RPT_ERR_UNSUPPORTED, "rpt_buffer_upsampled_image: built without the kernels");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipDeviceSynchronize());  // batches and planes may have been written on other streams
    const size_t n = size_t(b->width) * b->height, N = n * prm->scale * prm->scale;
    // mean 3 n, variance n, filtered mean 3 n (with a denoiser), the full-resolution frame 3 N, then its 3 N bytes
    HIP_TRY(b->d_up.reserve((7 * n + 3 * N) * 8 + 3 * N));
    double* const mean = b->d_up.get<double>();
    double* const var = mean + 3 * n;
    double* const up = mean + 7 * n;
    uint8_t* const img = reinterpret_cast<uint8_t*>(up + 3 * N);
    const double* lo = mean;
    if (int rc = rpt_buffer_mean_device(b, mean, var, nullptr)) return rc;
    if (d) {
        if (int rc = run_denoise(d, dprm, mean, var, static_cast<const double*>(d_lo_albedo), static_cast<const double*>(d_lo_normal),
                                 static_cast<const double*>(d_lo_depth), mean + 4 * n, nullptr, nullptr))
            return rc;
        lo = mean + 4 * n;
    }
    // (no variance is asked for, so none is read)
    if (int rc = run_upsample(prm, b->width, b->height, lo, nullptr, d_lo_albedo, d_lo_normal, d_lo_depth, d_hi_albedo, d_hi_normal, d_hi_depth,
                              up, nullptr, nullptr))
        return rc;
    HIP_TRY(launch_color_bytes(3 * N, up, img, nullptr));
    HIP_TRY(hipMemcpy(out_rgb8, img, 3 * N, hipMemcpyDeviceToHost));
    return RPT_OK;
}

// ---------------------------------------------------------------------------- temporal accumulation (temporal.hip)
int rpt_temporal_camera_record(const rpt_camera* cam, double out[13]) {
    if (!cam || !out) return fail(RPT_ERR_INVALID, "null argument");
    for (int i = 0; i < 3; i++)
        if (!std::isfinite(cam->eye[i]) || !std::isfinite(cam->direction[i]) || !std::isfinite(cam->up[i]))
            return fail(RPT_ERR_INVALID, "camera: a field is not finite");
    if (!std::isfinite(cam->fov) || !std::isfinite(cam->aperture) || !std::isfinite(cam->focal_distance))
        return fail(RPT_ERR_INVALID, "camera: a field is not finite");
    if (!(cam->fov > 0.0 && cam->fov < M_PI)) return fail(RPT_ERR_INVALID, "camera: fov must be in (0, pi)");
    const D3 c = cross(d3(cam->direction), d3(cam->up));
    const double l = std::sqrt((c.x * c.x + c.y * c.y) + c.z * c.z);
    if (!(l > 0.0) || std::isinf(l)) return fail(RPT_ERR_INVALID, "camera: direction and up have no cross product");
    for (int i = 0; i < 3; i++) {
        out[i] = cam->eye[i];
        out[3 + i] = cam->direction[i];
        out[6 + i] = comp(c, i) / l;
        out[9 + i] = cam->up[i];
    }
    out[12] = 1.0 / std::tan(cam->fov / 2.0);
    return RPT_OK;
}
struct rpt_temporal {
    int device = 0;
    uint32_t width = 0, height = 0;
    rpti::DevMem d_rec[2];             // the history: records of kTemporalRecDoubles doubles; d_rec[cur] is read, the other written
    int cur = 0;
    uint32_t frames = 0;               // since create / reset; 0: d_rec[cur] holds no frame
    TemporalCam cam{};                 // the record of the call that wrote d_rec[cur]
    rpti::DevMem d_host;               // rpt_temporal_accumulate: the planes of the host entry point
    rpti::DevMem d_frame;              // rpt_temporal_frame_image: mean, variance, accumulated frame and variance, filtered frame
    rpti::Event done;                  // recorded after the kernel of a call: the next call waits for it, whatever its stream
    bool used = false;
    // The one-shot motion table of the next call that passes its checks (motion_set: 0 none, 1 host records, 2 the caller's device table, 3 host
    // records that a preview has already uploaded to d_motion).
    int motion_set = 0;
    uint32_t n_motion = 0;
    std::vector<double> motion_host;   // rpt_temporal_set_motion's copy, uploaded by the consuming call on its stream
    std::vector<double> motion_sent;   // ... and the copy the last upload read (never the one a later set writes)
    const double* motion_dev = nullptr;  // rpt_temporal_set_motion_device's table
    rpti::DevMem d_motion;             // the uploaded table
    // rpt_temporal_set_clip's settings, read by a call with RPT_TEMPORAL_CLIP: a setting, kept over calls and resets
    uint32_t clip_radius = 1, clip_history = 1;
    double clip_gamma = 0.5;
};
rpt_temporal* rpt_temporal_create(int device, uint32_t width, uint32_t height) {
    if (width == 0 || height == 0 || uint64_t(width) * height >= (1ull << 31)) { fail(RPT_ERR_INVALID, "bad accumulator size"); return nullptr; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { fail(RPT_ERR_INVALID, "device index out of range"); return nullptr; }
    auto* t = new rpt_temporal();
    t->device = device;
    t->width = width;
    t->height = height;
    const size_t bytes = size_t(width) * height * kTemporalRecDoubles * sizeof(double);
    const bool ok = hipSetDevice(device) == hipSuccess && t->d_rec[0].reserve(bytes) == hipSuccess && t->d_rec[1].reserve(bytes) == hipSuccess &&
                    t->done.create(hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        fail(RPT_ERR_DEVICE, "rpt_temporal_create: device allocation failed");
        rpt_temporal_destroy(t);
        return nullptr;
    }
    return t;
}
void rpt_temporal_destroy(rpt_temporal* t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    delete t;
}
int rpt_temporal_reset(rpt_temporal* t) {
    if (!t) return fail(RPT_ERR_INVALID, "null accumulator");
    t->frames = 0;                     // the next call looks nothing up; what the arrays hold is never read
    t->motion_set = 0;                 // a table that was not consumed belongs to the sequence that ends here
    return RPT_OK;
}
int rpt_temporal_frames(rpt_temporal* t, uint32_t* n) {
    if (!t || !n) return fail(RPT_ERR_INVALID, "null argument");
    *n = t->frames;
    return RPT_OK;
}
// The nine cofactors k (the adjugate: inverse = k / det) and the determinant of a 3 x 3 matrix m, in the order include/rpt_hip.h states.
static double cofactors3(const double m[3][3], double k[3][3]) {
    k[0][0] = m[1][1] * m[2][2] - m[1][2] * m[2][1]; k[0][1] = m[0][2] * m[2][1] - m[0][1] * m[2][2]; k[0][2] = m[0][1] * m[1][2] - m[0][2] * m[1][1];
    k[1][0] = m[1][2] * m[2][0] - m[1][0] * m[2][2]; k[1][1] = m[0][0] * m[2][2] - m[0][2] * m[2][0]; k[1][2] = m[0][2] * m[1][0] - m[0][0] * m[1][2];
    k[2][0] = m[1][0] * m[2][1] - m[1][1] * m[2][0]; k[2][1] = m[0][1] * m[2][0] - m[0][0] * m[2][1]; k[2][2] = m[0][0] * m[1][1] - m[0][1] * m[1][0];
    return (m[0][0] * k[0][0] + m[0][1] * k[1][0]) + m[0][2] * k[2][0];
}
// (No operation below may be contracted into an fma: the pragma above check_scene64 holds to the end of the file.)
int rpt_temporal_motion_record(const double cur[16], const double prev[16], double out[24]) {
    if (!cur || !prev || !out) return fail(RPT_ERR_INVALID, "null argument");
    bool same = true;
    for (int i = 0; i < 16; i++) {
        if (!std::isfinite(cur[i]) || !std::isfinite(prev[i])) return fail(RPT_ERR_INVALID, "motion record: a matrix value is not finite");
        same = same && cur[i] == prev[i];
    }
    for (const double* m : {cur, prev})
        if (m[12] != 0.0 || m[13] != 0.0 || m[14] != 0.0 || m[15] != 1.0) return fail(RPT_ERR_INVALID, "motion record: the bottom row must be 0 0 0 1");
    double c[3][3], k[3][3], a[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) c[i][j] = cur[4 * i + j];
    const double det = cofactors3(c, k);
    if (det == 0.0 || !std::isfinite(det)) return fail(RPT_ERR_INVALID, "motion record: the current matrix has no inverse");
    for (int i = 0; i < 24; i++) out[i] = 0.0;
    if (same) {
        out[0] = out[5] = out[10] = out[12] = out[16] = out[20] = 1.0;
        return RPT_OK;
    }
    double inv[3][3], u[3];
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) inv[i][j] = k[i][j] / det;
        u[i] = -((inv[i][0] * cur[3] + inv[i][1] * cur[7]) + inv[i][2] * cur[11]);
    }
    for (int i = 0; i < 3; i++) {
        const double* const p = prev + 4 * i;
        for (int j = 0; j < 3; j++) a[i][j] = out[4 * i + j] = (p[0] * inv[0][j] + p[1] * inv[1][j]) + p[2] * inv[2][j];
        out[4 * i + 3] = ((p[0] * u[0] + p[1] * u[1]) + p[2] * u[2]) + p[3];
    }
    const double det_a = cofactors3(a, k);
    if (det_a == 0.0 || !std::isfinite(det_a)) {
        for (int i = 0; i < 24; i++) out[i] = 0.0;
        return fail(RPT_ERR_INVALID, "motion record: the map between the frames has no inverse");
    }
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) out[12 + 3 * i + j] = k[j][i] / det_a;
    return RPT_OK;
}
int rpt_temporal_set_motion(rpt_temporal* t, const double* records, uint32_t n_objects) {
    if (!records && n_objects) return fail(RPT_ERR_INVALID, "null motion records");
    for (size_t o = 0; o < n_objects; o++)
        for (int i = 0; i < 21; i++)
            if (!std::isfinite(records[o * kTemporalMotionDoubles + i])) return fail(RPT_ERR_INVALID, "motion records: a value is not finite");
    if (!t) return fail(RPT_ERR_INVALID, "null accumulator");
    t->motion_set = n_objects ? 1 : 0;
    t->n_motion = n_objects;
    t->motion_host.assign(records, records + size_t(n_objects) * kTemporalMotionDoubles);
    return RPT_OK;
}
int rpt_temporal_set_motion_device(rpt_temporal* t, const void* d_records, uint32_t n_objects) {
    if (!d_records && n_objects) return fail(RPT_ERR_INVALID, "null motion records");
    if (!t) return fail(RPT_ERR_INVALID, "null accumulator");
    t->motion_set = n_objects ? 2 : 0;
    t->n_motion = n_objects;
    t->motion_dev = static_cast<const double*>(d_records);
    return RPT_OK;
}
int rpt_temporal_set_clip(rpt_temporal* t, uint32_t radius, double gamma, uint32_t clip_history) {
    if (radius < 1 || radius > kTemporalClipMaxRadius) return fail(RPT_ERR_INVALID, "clip radius must be 1..3");
    if (!(gamma >= 0.0) || std::isinf(gamma)) return fail(RPT_ERR_INVALID, "clip gamma must be finite and >= 0");
    if (clip_history > 4096) return fail(RPT_ERR_INVALID, "clip_history must be 0..4096 (0: a clipped pixel keeps its length)");
    if (!t) return fail(RPT_ERR_INVALID, "null accumulator");
    t->clip_radius = radius;
    t->clip_gamma = gamma;
    t->clip_history = clip_history;
    return RPT_OK;
}
// What rpt_temporal_* refuse before any device call; the call's camera record to *rec.
static int check_temporal(const rpt_temporal* t, const rpt_temporal_params* prm, const rpt_camera* cam, const void* rgb, const void* var,
                          const void* normal, const void* depth, const void* out, const void* out_var, const void* out_len, TemporalCam* rec,
                          bool null_tile_list = false /* a preview's d_tiles == NULL with n_tiles > 0 */) {
    if (!prm) return fail(RPT_ERR_INVALID, "null temporal parameters");
    if (prm->max_history < 1 || prm->max_history > 4096) return fail(RPT_ERR_INVALID, "max_history must be 1..4096");
    if (prm->flags & ~(RPT_TEMPORAL_MATCH_ID | RPT_TEMPORAL_CLIP)) return fail(RPT_ERR_INVALID, "unknown temporal flag");
    for (double tol : {prm->depth_tol, prm->normal_tol})
        if (!(tol >= 0.0) || std::isinf(tol)) return fail(RPT_ERR_INVALID, "a tolerance must be finite and >= 0 (0: the test is off)");
    if (!cam) return fail(RPT_ERR_INVALID, "null camera");
    static_assert(sizeof(TemporalCam) == 13 * sizeof(double), "the camera record is 13 doubles");
    if (int rc = rpt_temporal_camera_record(cam, reinterpret_cast<double*>(rec))) return rc;
    if (!rgb || !out) return fail(RPT_ERR_INVALID, "null frame");
    if (!depth) return fail(RPT_ERR_INVALID, "the accumulation needs the depth plane");
    if (prm->normal_tol > 0.0 && !normal) return fail(RPT_ERR_INVALID, "normal_tol > 0 needs the normal plane");
    if (!(prm->normal_tol > 0.0) && normal) return fail(RPT_ERR_INVALID, "normal_tol == 0 takes no normal plane");
    for (const void* o : {out, out_var, out_len})
        for (const void* in : {rgb, var, normal, depth})
            if (o && o == in) return fail(RPT_ERR_INVALID, "an output must not be one of the inputs");
    if (out == out_var || out == out_len || (out_var && out_var == out_len)) return fail(RPT_ERR_INVALID, "the outputs must differ");
    if (null_tile_list) return fail(RPT_ERR_INVALID, "null tile list");
    // (with RPT_TEMPORAL_CLIP the call would read its three settings from the accumulator: the refusal names the flag that needs them)
    if (!t) return fail(RPT_ERR_INVALID, (prm->flags & RPT_TEMPORAL_CLIP) ? "null accumulator: the flag RPT_TEMPORAL_CLIP reads its settings from it" : "null accumulator");
    return RPT_OK;
}
// (The arguments have passed check_temporal.)  preview: rpt_temporal_preview_device over d_tiles / n_tiles -- ordered through the same
// event, the same arguments, the same table, but nothing of the accumulator's changes: no record is written, the records do not swap,
// the camera record and the frame count stay, and the motion table stays set.  A host table is uploaded by the first call that reads
// it, preview or not (motion_set 1 -> 3: "host records, already in d_motion"); the calls behind it wait for that call's event.
static int run_temporal(rpt_temporal* t, const rpt_temporal_params* prm, const TemporalCam& rec, const double* d_rgb, const double* d_var,
                        const double* d_normal, const double* d_depth, double* d_out, double* d_out_var, double* d_out_len, hipStream_t st,
                        bool preview = false, const uint32_t* d_tiles = nullptr, uint32_t n_tiles = 0) {
    if (!launch_temporal_accumulate) return fail(RPT_ERR_UNSUPPORTED, "rpt_temporal_accumulate: built without the kernels");
    if (preview && !launch_temporal_preview) return fail(RPT_ERR_UNSUPPORTED, "rpt_temporal_preview_device: built without the kernels");
    HIP_TRY(hipSetDevice(t->device));
    if (t->used) HIP_TRY(hipStreamWaitEvent(st, t->done.get(), 0));
    t->used = true;
    TemporalArgs a{};
    a.width = t->width; a.height = t->height; a.max_history = prm->max_history; a.flags = prm->flags;
    a.have_history = t->frames ? 1u : 0u;
    a.depth_tol = prm->depth_tol; a.normal_tol = prm->normal_tol;
    a.cur = rec;
    a.prev = t->cam;
    a.rgb = d_rgb; a.var = d_var; a.normal = d_normal; a.depth = d_depth;
    a.hist_in = t->d_rec[t->cur].get<double>();
    a.hist_out = t->d_rec[t->cur ^ 1].get<double>();
    a.out_rgb = d_out; a.out_var = d_out_var; a.out_len = d_out_len;
    if (prm->flags & RPT_TEMPORAL_CLIP) {
        a.clip_radius = t->clip_radius; a.clip_gamma = t->clip_gamma; a.clip_history = t->clip_history;
    }
    if (t->motion_set == 1) {
        // behind the predecessor's event on this call's stream: the kernel of an earlier call may still be reading d_motion
        if (!launch_temporal_motion_upload) return fail(RPT_ERR_UNSUPPORTED, "rpt_temporal_set_motion: built without the kernels");
        const size_t bytes = size_t(t->n_motion) * kTemporalMotionDoubles * sizeof(double);
        HIP_TRY(t->d_motion.reserve(bytes));
        t->motion_sent.swap(t->motion_host);
        if (hipError_t e = launch_temporal_motion_upload(t->d_motion.get(), t->motion_sent.data(), bytes, st); e != hipSuccess) {
            t->motion_sent.swap(t->motion_host);   // the table stays set for the next call
            return fail(RPT_ERR_DEVICE, std::string("the motion table's upload: ") + hipGetErrorString(e));
        }
        a.motion = t->d_motion.get<double>();
        t->motion_set = 3;
    } else if (t->motion_set == 2) {
        a.motion = t->motion_dev;
    } else if (t->motion_set == 3) {
        a.motion = t->d_motion.get<double>();
    }
    a.n_motion = a.motion ? t->n_motion : 0u;
    if (preview) {
        HIP_TRY(launch_temporal_preview(a, d_tiles, n_tiles, st));
        HIP_TRY(hipEventRecord(t->done.get(), st));
        return RPT_OK;
    }
    t->motion_set = 0;                 // one-shot: the table describes this frame's motion only
    HIP_TRY(launch_temporal_accumulate(a, st));
    HIP_TRY(hipEventRecord(t->done.get(), st));
    t->cur ^= 1;
    t->cam = rec;
    if (t->frames != 0xFFFFFFFFu) t->frames++;
    return RPT_OK;
}
int rpt_temporal_accumulate_device(rpt_temporal* t, const rpt_temporal_params* prm, const rpt_camera* cam, const void* d_rgb, const void* d_var,
                                   const void* d_normal, const void* d_depth, void* d_out_rgb, void* d_out_var, void* d_out_len,
                                   void* hip_stream) {
    TemporalCam rec;
    if (int rc = check_temporal(t, prm, cam, d_rgb, d_var, d_normal, d_depth, d_out_rgb, d_out_var, d_out_len, &rec)) return rc;
    return run_temporal(t, prm, rec, static_cast<const double*>(d_rgb), static_cast<const double*>(d_var), static_cast<const double*>(d_normal),
                        static_cast<const double*>(d_depth), static_cast<double*>(d_out_rgb), static_cast<double*>(d_out_var),
                        static_cast<double*>(d_out_len), static_cast<hipStream_t>(hip_stream));
}
int rpt_temporal_preview_device(rpt_temporal* t, const rpt_temporal_params* prm, const rpt_camera* cam, const void* d_rgb, const void* d_var,
                                const void* d_normal, const void* d_depth, const void* d_tiles, uint32_t n_tiles, void* d_out_rgb, void* d_out_var,
                                void* d_out_len, void* hip_stream) {
    TemporalCam rec;
    if (int rc = check_temporal(t, prm, cam, d_rgb, d_var, d_normal, d_depth, d_out_rgb, d_out_var, d_out_len, &rec, !d_tiles && n_tiles)) return rc;
    if (d_tiles && n_tiles > ((t->width + 31u) / 32u) * ((t->height + 31u) / 32u))
        return fail(RPT_ERR_INVALID, "rpt_temporal_preview_device: more tiles listed than the frame has (the ids of a list are distinct)");
    return run_temporal(t, prm, rec, static_cast<const double*>(d_rgb), static_cast<const double*>(d_var), static_cast<const double*>(d_normal),
                        static_cast<const double*>(d_depth), static_cast<double*>(d_out_rgb), static_cast<double*>(d_out_var),
                        static_cast<double*>(d_out_len), static_cast<hipStream_t>(hip_stream), true, static_cast<const uint32_t*>(d_tiles), n_tiles);
}
int rpt_temporal_tile_errors_device(rpt_temporal* t, const void* d_rgb, const void* d_var, double floor, const void* d_tiles, uint32_t n_tiles,
                                    void* d_err, void* hip_stream) {
    if (!(floor > 0.0) || std::isinf(floor)) return fail(RPT_ERR_INVALID, "floor must be finite and > 0");
    if (!t || !d_rgb || !d_var || !d_err) return fail(RPT_ERR_INVALID, "null argument");
    if (!d_tiles && n_tiles) return fail(RPT_ERR_INVALID, "null tile list");
    if (d_tiles && n_tiles > ((t->width + 31u) / 32u) * ((t->height + 31u) / 32u))
        return fail(RPT_ERR_INVALID, "rpt_temporal_tile_errors_device: more tiles listed than the frame has (the ids of a list are distinct)");
    if (!launch_plane_tile_errors) return fail(RPT_ERR_UNSUPPORTED, "rpt_temporal_tile_errors_device: built without the kernels");
    HIP_TRY(hipSetDevice(t->device));
    HIP_TRY(launch_plane_tile_errors(t->width, t->height, floor, static_cast<const double*>(d_rgb), static_cast<const double*>(d_var),
                                     static_cast<const uint32_t*>(d_tiles), n_tiles, static_cast<double*>(d_err), static_cast<hipStream_t>(hip_stream)));
    return RPT_OK;
}
int rpt_render_adaptive_temporal(rpt_scene* s, const rpt_camera* cam, const rpt_render_params* prm, const rpt_adaptive_params* p, uint64_t seed,
                                 uint32_t sample_offset, rpt_buffer* b, rpt_temporal* t, const rpt_temporal_params* tprm, const void* d_normal,
                                 const void* d_depth, uint64_t stats[4]) {
    if (!s || !cam || !prm) return fail(RPT_ERR_INVALID, "null argument");
    if (int rc = check_adaptive(p)) return rc;
    if (uint64_t(sample_offset) + uint64_t(p->max_batches) * p->spp_per_batch > 0xFFFFFFFFull)
        return fail(RPT_ERR_INVALID, "sample_offset + max_batches * spp_per_batch must fit 32 bits");
    if (prm->shard_count > 1) return fail(RPT_ERR_INVALID, "an adaptive render is not sharded");
    if (!b) return fail(RPT_ERR_INVALID, "null buffer");
    if (prm->width != b->width || prm->height != b->height) return fail(RPT_ERR_INVALID, "Invalid sample dimension");  // buffer.rs:33-36
    if (s->committed && s->device != b->device) return fail(RPT_ERR_INVALID, "buffer and scene live on different devices");
    // (the frame, its variance and the preview come from the buffer and the accumulator: placeholders that are no plane of the
    // caller's.  The accumulation reads the normal plane only where its test is on.)
    TemporalCam rec;
    const void* const t_normal = tprm && tprm->normal_tol > 0.0 ? d_normal : nullptr;
    if (int rc = check_temporal(t, tprm, cam, &rec, nullptr, t_normal, d_depth, b, nullptr, nullptr, &rec)) return rc;
    if (b->device != t->device) return fail(RPT_ERR_INVALID, "buffer and accumulator live on different devices");
    if (b->width != t->width || b->height != t->height) return fail(RPT_ERR_INVALID, "buffer and accumulator have different sizes");
    if (b->n_batches || b->d_extra) return fail(RPT_ERR_STATE, "rpt_render_adaptive_temporal needs an empty buffer");
    if (!launch_buffer_mean || !launch_temporal_preview || !launch_plane_tile_errors || !launch_tile_select_list)
        return fail(RPT_ERR_UNSUPPORTED, "rpt_render_adaptive_temporal: built without the kernels");
    for (uint32_t k = 0; k < p->min_batches; k++)
        if (int rc = rpt_render_into_buffer(s, cam, prm, p->spp_per_batch, seed, sample_offset + k * p->spp_per_batch, b)) return rc;
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipDeviceSynchronize());  // the planes may have been written on other streams
    const size_t n = size_t(b->width) * b->height;
    HIP_TRY(b->d_active.reserve(size_t(b->n_tiles()) * 4));
    HIP_TRY(b->d_tile_err.reserve(size_t(b->n_tiles()) * 8 + 8));
    HIP_TRY(t->d_frame.reserve(11 * n * 8));  // (rpt_temporal_frame_image's size: the frame's last call will ask for it)
    uint32_t* const d_active = b->d_active.get<uint32_t>();
    double* const err = b->d_tile_err.get<double>();
    uint32_t* const d_count = reinterpret_cast<uint32_t*>(err + b->n_tiles());
    double* const mean = t->d_frame.get<double>();
    double* const var = mean + 3 * n;
    double* const acc = mean + 4 * n;
    double* const acc_var = mean + 7 * n;
    uint64_t rounds = 0, tile_batches = uint64_t(p->min_batches) * b->n_tiles();
    // The active list starts as every tile (a null list) and only shrinks: a tile that left it is not evaluated again.
    const uint32_t* list = nullptr;
    uint32_t n_active = 0;
    for (uint32_t k = p->min_batches; k < p->max_batches; k++) {
        if (int rc = rpt_buffer_mean_device(b, mean, var, nullptr)) return rc;
        if (int rc = run_temporal(t, tprm, rec, mean, var, static_cast<const double*>(t_normal), static_cast<const double*>(d_depth), acc, acc_var,
                                  nullptr, nullptr, true, list, n_active))
            return rc;
        HIP_TRY(launch_plane_tile_errors(b->width, b->height, p->floor, acc, acc_var, list, n_active, err, nullptr));
        HIP_TRY(launch_tile_select_list(b->view(), p->threshold * p->threshold, p->max_batches, err, list, n_active, d_active, d_count, nullptr));
        HIP_TRY(hipStreamSynchronize(nullptr));   // the one synchronisation and the one read-back of a round, 4 bytes
        HIP_TRY(hipMemcpy(&n_active, d_count, 4, hipMemcpyDeviceToHost));
        list = d_active;
        if (n_active == 0) break;
        if (int rc = rpt_render_sample_tiles_device(s, cam, prm, p->spp_per_batch, seed, sample_offset + k * p->spp_per_batch, d_active, n_active,
                                                    b->d_stage.get(), nullptr))
            return rc;
        if (int rc = rpt_buffer_add_samples_tiles_device(b, b->d_stage.get(), d_active, n_active, nullptr)) return rc;
        rounds++;
        tile_batches += n_active;
    }
    if (stats) {
        std::vector<uint32_t> nb(b->n_tiles());
        if (int rc = rpt_buffer_tile_batches(b, nb.data(), nb.size())) return rc;
        stats[0] = rounds;
        stats[1] = tile_batches;
        stats[2] = uint64_t(std::count(nb.begin(), nb.end(), p->max_batches));
        stats[3] = b->n_tiles();
    }
    return RPT_OK;
}
int rpt_temporal_accumulate(rpt_temporal* t, const rpt_temporal_params* prm, const rpt_camera* cam, const double* rgb, const double* var,
                            const double* normal, const double* depth, double* out_rgb, double* out_var, double* out_len) {
    TemporalCam rec;
    if (int rc = check_temporal(t, prm, cam, rgb, var, normal, depth, out_rgb, out_var, out_len, &rec)) return rc;
    HIP_TRY(hipSetDevice(t->device));
    const size_t n = size_t(t->width) * t->height;
    // rgb, normal, depth, out: 3 n each; var, out_var, out_len: n each
    HIP_TRY(t->d_host.reserve(15 * n * 8));
    double* const base = t->d_host.get<double>();
    const double* const ins[4] = {rgb, normal, depth, var};
    double* dev[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int k = 0; k < 4; k++)
        if (ins[k]) {
            dev[k] = base + size_t(k) * 3 * n;
            HIP_TRY(hipMemcpy(dev[k], ins[k], (k == 3 ? n : 3 * n) * 8, hipMemcpyHostToDevice));
        }
    double* const d_out = base + 10 * n;
    double* const d_out_var = out_var ? base + 13 * n : nullptr;
    double* const d_out_len = out_len ? base + 14 * n : nullptr;
    if (int rc = run_temporal(t, prm, rec, dev[0], dev[3], dev[1], dev[2], d_out, d_out_var, d_out_len, nullptr)) return rc;
    HIP_TRY(hipMemcpy(out_rgb, d_out, 3 * n * 8, hipMemcpyDeviceToHost));
    if (out_var) HIP_TRY(hipMemcpy(out_var, d_out_var, n * 8, hipMemcpyDeviceToHost));
    if (out_len) HIP_TRY(hipMemcpy(out_len, d_out_len, n * 8, hipMemcpyDeviceToHost));
    return RPT_OK;
}
int rpt_temporal_frame_image(rpt_temporal* t, const rpt_temporal_params* prm, const rpt_camera* cam, rpt_buffer* b, rpt_denoiser* d,
                             const rpt_denoise_params* dprm, const void* d_albedo, const void* d_normal, const void* d_depth,
                             uint8_t* out_rgb8) {
    // (the frame and its variance come from the buffer, the accumulated ones from the accumulator: placeholders that are no plane of
    // the caller's.  The accumulation reads the normal plane only where its test is on.)
    TemporalCam rec;
    const void* const t_normal = prm && prm->normal_tol > 0.0 ? d_normal : nullptr;
    if (int rc = check_temporal(t, prm, cam, &rec, nullptr, t_normal, d_depth, out_rgb8, nullptr, nullptr, &rec)) return rc;
    if (d)
        if (int rc = check_denoise(d, dprm, &rec, dprm && dprm->sigma_color > 0.0 ? t : nullptr, d_albedo, d_normal, d_depth, out_rgb8, nullptr)) return rc;
    if (!b) return fail(RPT_ERR_INVALID, "null buffer");
    if (b->device != t->device || (d && d->device != t->device)) return fail(RPT_ERR_INVALID, "buffer, denoiser and accumulator live on different devices");
    if (b->width != t->width || b->height != t->height || (d && (d->width != t->width || d->height != t->height)))
        return fail(RPT_ERR_INVALID, "buffer, denoiser and accumulator have different sizes");
    if (b->n_batches < 2) return fail(RPT_ERR_STATE, "the variance of the mean needs at least 2 batches");
    if (!launch_buffer_mean || !launch_color_bytes || !launch_temporal_accumulate)
        return fail(RPT_ERR_UNSUPPORTED, "rpt_temporal_frame_image: built without the kernels");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipDeviceSynchronize());  // batches and planes may have been written on other streams
    const size_t n = size_t(b->width) * b->height;
    HIP_TRY(t->d_frame.reserve(11 * n * 8));
    double* const mean = t->d_frame.get<double>();
    double* const var = mean + 3 * n;
    double* const acc = mean + 4 * n;
    double* const acc_var = mean + 7 * n;
    double* out = acc;
    if (int rc = rpt_buffer_mean_device(b, mean, var, nullptr)) return rc;
    if (int rc = run_temporal(t, prm, rec, mean, var, static_cast<const double*>(t_normal), static_cast<const double*>(d_depth), acc, acc_var,
                              nullptr, nullptr))
        return rc;
    if (d) {
        out = mean + 8 * n;
        if (int rc = run_denoise(d, dprm, acc, acc_var, static_cast<const double*>(d_albedo), static_cast<const double*>(d_normal),
                                 static_cast<const double*>(d_depth), out, nullptr, nullptr))
            return rc;
    }
    HIP_TRY(launch_color_bytes(3 * n, out, b->d_img.get<uint8_t>(), nullptr));
    HIP_TRY(hipMemcpy(out_rgb8, b->d_img.get(), n * 3, hipMemcpyDeviceToHost));
    return RPT_OK;
}

int rpt_get_timing(rpt_scene* s, double* render_ms, double* resolve_ms, int32_t* grid_blocks) {
    if (!s) return fail(RPT_ERR_INVALID, "null scene");
    if (!s->ev_count) return fail(RPT_ERR_STATE, "no timed render: rpt_set_option(\"timing\", 1) first");
    const rpti::Event* ev = &s->dev.evs[3 * ((s->ev_count - 1) % rpt_scene::kTimedLaunches)];
    HIP_TRY(hipEventSynchronize(ev[2].get()));
    float a = 0.f, b = 0.f;
    HIP_TRY(hipEventElapsedTime(&a, ev[0].get(), ev[1].get()));
    HIP_TRY(hipEventElapsedTime(&b, ev[1].get(), ev[2].get()));
    if (render_ms) *render_ms = a;
    if (resolve_ms) *resolve_ms = b;
    if (grid_blocks) *grid_blocks = s->last_blocks;
    return RPT_OK;
}

int rpt_get_timing_mean(rpt_scene* s, double* render_ms, double* resolve_ms, int32_t* launches) {
    if (!s) return fail(RPT_ERR_INVALID, "null scene");
    if (!s->ev_count) return fail(RPT_ERR_STATE, "no timed render: rpt_set_option(\"timing\", 1) first");
    const size_t n = std::min(s->ev_count, rpt_scene::kTimedLaunches);  // the ring keeps the latest launches
    HIP_TRY(hipEventSynchronize(s->dev.evs[3 * ((s->ev_count - 1) % rpt_scene::kTimedLaunches) + 2].get()));
    double a = 0.0, b = 0.0;
    for (size_t i = 0; i < n; i++) {
        const rpti::Event* ev = &s->dev.evs[3 * i];
        float x = 0.f, y = 0.f;
        HIP_TRY(hipEventElapsedTime(&x, ev[0].get(), ev[1].get()));
        HIP_TRY(hipEventElapsedTime(&y, ev[1].get(), ev[2].get()));
        a += x;
        b += y;
    }
    if (render_ms) *render_ms = a / double(n);
    if (resolve_ms) *resolve_ms = b / double(n);
    if (launches) *launches = int32_t(n);
    s->ev_count = 0;
    return RPT_OK;
}

int rpt_scene_stats(rpt_scene* s, uint64_t out[16]) {
    if (!s || !out) return fail(RPT_ERR_INVALID, "null argument");
    if (!s->committed) return fail(RPT_ERR_STATE, "rpt_scene_commit must be called first");
    std::memcpy(out, s->stats, sizeof(s->stats));
    return RPT_OK;
}

int rpt_get_counters(rpt_scene* s, uint64_t out[8]) {
    if (!s || !out) return fail(RPT_ERR_INVALID, "null argument");
    std::memcpy(out, s->last_counters, 64);
    return RPT_OK;
}
int rpt_debug_section_counters(rpt_scene* s, uint64_t out[56]) {
    if (!s || !out) return fail(RPT_ERR_INVALID, "null argument");
    std::memcpy(out, s->last_counters + 8, 56 * 8);
    return RPT_OK;
}

int rpt_scan_cull_counters(rpt_scene* s, uint64_t out[16]) {
    if (!s || !out) return fail(RPT_ERR_INVALID, "null argument");
    if (!s->committed) return fail(RPT_ERR_STATE, "rpt_scene_commit must be called first");
    for (int i = 0; i < 12; i++) out[i] = s->last_cull[i];
    const SceneView& v = s->view;
    const bool eligible = !(v.scan_bound.lo[0] > v.scan_bound.hi[0]);
    out[12] = eligible ? 1 : 0;
    out[13] = v.n_scan_groups;
    out[14] = v.scan_always;
    out[15] = v.scan_cull;
    return RPT_OK;
}
int rpt_scan_cull_groups(rpt_scene* s, float out_boxes[36], uint64_t out_masks[5], uint32_t* n_groups, uint32_t* enabled) {
    if (!s || !out_boxes || !out_masks || !n_groups || !enabled) return fail(RPT_ERR_INVALID, "null argument");
    if (!s->committed) return fail(RPT_ERR_STATE, "rpt_scene_commit must be called first");
    const SceneView& v = s->view;
    for (int a = 0; a < 3; a++) { out_boxes[a] = v.scan_bound.lo[a]; out_boxes[3 + a] = v.scan_bound.hi[a]; }
    for (int a = 0; a < 3; a++) { out_boxes[30 + a] = v.scan_tail.lo[a]; out_boxes[33 + a] = v.scan_tail.hi[a]; }
    for (uint32_t g = 0; g < kMaxScanGroups; g++) {
        for (int a = 0; a < 3; a++) { out_boxes[6 + 6 * g + a] = v.scan_groups[g].box.lo[a]; out_boxes[9 + 6 * g + a] = v.scan_groups[g].box.hi[a]; }
        out_masks[g] = v.scan_groups[g].mask;
    }
    out_masks[4] = v.scan_always;
    *n_groups = v.n_scan_groups;
    *enabled = v.scan_cull;
    return RPT_OK;
}

// ---------------------------------------------------------------------------- test hooks
// Device scratch of one hook call, at least 16 bytes (an empty batch still gets a valid pointer).
static hipError_t hook_scratch(rpti::DevMem& m, size_t bytes) { return m.reserve(std::max<size_t>(bytes, 16)); }
int rpt_intersect_batch(rpt_scene* s, uint64_t n, const float* origins, const float* dirs, float* t, int32_t* object,
                        float* normal) {
    if (!s || !origins || !dirs || !t || !object) return fail(RPT_ERR_INVALID, "null argument");
    if (!s->committed) return fail(RPT_ERR_STATE, "rpt_scene_commit must be called first");
    if (n == 0) return RPT_OK;
    HIP_TRY(hipSetDevice(s->device));
    rpti::DevMem d_o, d_d, d_t, d_n, d_obj;
    HIP_TRY(hook_scratch(d_o, n * 12));
    HIP_TRY(hook_scratch(d_d, n * 12));
    HIP_TRY(hook_scratch(d_t, n * 4));
    HIP_TRY(hook_scratch(d_n, n * 12));
    HIP_TRY(hook_scratch(d_obj, n * 4));
    HIP_TRY(hipMemcpy(d_o.get(), origins, n * 12, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_d.get(), dirs, n * 12, hipMemcpyHostToDevice));
    if (int rc = rpti::wait_for_move(s, nullptr)) return rc;
    HIP_TRY(launch_intersect(s->view, n, d_o.get<float>(), d_d.get<float>(), d_t.get<float>(), d_obj.get<int32_t>(), d_n.get<float>(),
                             s->view.n_nodes != 0, nullptr));
    HIP_TRY(hipMemcpy(t, d_t.get(), n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(object, d_obj.get(), n * 4, hipMemcpyDeviceToHost));
    if (normal) HIP_TRY(hipMemcpy(normal, d_n.get(), n * 12, hipMemcpyDeviceToHost));
    return RPT_OK;
}

int rpt_intersect_segments(rpt_scene* s, uint64_t n, const float* origins, const float* dirs, const float* t_max, float* t, uint32_t* code) {
    if (!s || !origins || !dirs || !t_max || !t || !code) return fail(RPT_ERR_INVALID, "null argument");
    if (!s->committed) return fail(RPT_ERR_STATE, "rpt_scene_commit must be called first");
    if (s->view.n_nodes != 0 || s->view.scene_bvh || s->view.n_mono || s->view.n_inst)
        return fail(RPT_ERR_UNSUPPORTED, "rpt_intersect_segments: the scene has a tree or monomial surfaces (the query is the linear scan's)");
    if (!launch_intersect_segments) return fail(RPT_ERR_UNSUPPORTED, "rpt_intersect_segments: built without the kernels");
    if (n == 0) return RPT_OK;
    HIP_TRY(hipSetDevice(s->device));
    rpti::DevMem d_o, d_d, d_m, d_t, d_c;
    HIP_TRY(hook_scratch(d_o, n * 12));
    HIP_TRY(hook_scratch(d_d, n * 12));
    HIP_TRY(hook_scratch(d_m, n * 4));
    HIP_TRY(hook_scratch(d_t, n * 4));
    HIP_TRY(hook_scratch(d_c, n * 4));
    HIP_TRY(hipMemcpy(d_o.get(), origins, n * 12, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_d.get(), dirs, n * 12, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_m.get(), t_max, n * 4, hipMemcpyHostToDevice));
    if (int rc = rpti::wait_for_move(s, nullptr)) return rc;
    HIP_TRY(launch_intersect_segments(s->view, n, d_o.get<float>(), d_d.get<float>(), d_m.get<float>(), d_t.get<float>(), d_c.get<uint32_t>(), nullptr));
    HIP_TRY(hipMemcpy(t, d_t.get(), n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(code, d_c.get(), n * 4, hipMemcpyDeviceToHost));
    return RPT_OK;
}

int rpt_debug_rng_u32(uint64_t seed, uint32_t pixel, uint32_t sample, uint32_t n, uint32_t* out) {
    if (!out) return fail(RPT_ERR_INVALID, "null argument");
    rpti::DevMem d;
    HIP_TRY(hook_scratch(d, size_t(n) * 4));
    HIP_TRY(launch_debug_rng(seed_mix(seed), pixel, sample, n, d.get<uint32_t>(), nullptr));
    HIP_TRY(hipMemcpy(out, d.get(), size_t(n) * 4, hipMemcpyDeviceToHost));
    return RPT_OK;
}
static Material to_gpu_material(const rpt_material* m) {
    Material g;
    g.albedo_emit = F4{float(m->albedo[0]), float(m->albedo[1]), float(m->albedo[2]), float(m->emittance)};
    g.params = F4{bits_f(uint32_t(m->kind)), float(m->shininess), float(m->ior), 0.f};
    return g;
}
int rpt_debug_material_sample_f(const rpt_material* m, uint64_t n, const float* normals, const float* wos, uint64_t seed,
                                float* wi, float* pdf, int32_t* some) {
    std::string why;
    if (!check_material(m, why) || !normals || !wos || !wi || !pdf || !some) return fail(RPT_ERR_INVALID, "bad argument");
    rpti::DevMem d_n, d_wo, d_wi, d_pdf, d_some;
    HIP_TRY(hook_scratch(d_n, n * 12));
    HIP_TRY(hook_scratch(d_wo, n * 12));
    HIP_TRY(hook_scratch(d_wi, n * 12));
    HIP_TRY(hook_scratch(d_pdf, n * 4));
    HIP_TRY(hook_scratch(d_some, n * 4));
    HIP_TRY(hipMemcpy(d_n.get(), normals, n * 12, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_wo.get(), wos, n * 12, hipMemcpyHostToDevice));
    HIP_TRY(launch_debug_sample_f(to_gpu_material(m), n, d_n.get<float>(), d_wo.get<float>(), seed_mix(seed), d_wi.get<float>(), d_pdf.get<float>(),
                                  d_some.get<int32_t>(), nullptr));
    HIP_TRY(hipMemcpy(wi, d_wi.get(), n * 12, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(pdf, d_pdf.get(), n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(some, d_some.get(), n * 4, hipMemcpyDeviceToHost));
    return RPT_OK;
}
int rpt_debug_material_bsdf(const rpt_material* m, uint64_t n, const float* normals, const float* wos, const float* wis,
                            float* out_rgb) {
    std::string why;
    if (!check_material(m, why) || !normals || !wos || !wis || !out_rgb) return fail(RPT_ERR_INVALID, "bad argument");
    rpti::DevMem d_n, d_wo, d_wi, d_out;
    HIP_TRY(hook_scratch(d_n, n * 12));
    HIP_TRY(hook_scratch(d_wo, n * 12));
    HIP_TRY(hook_scratch(d_wi, n * 12));
    HIP_TRY(hook_scratch(d_out, n * 12));
    HIP_TRY(hipMemcpy(d_n.get(), normals, n * 12, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_wo.get(), wos, n * 12, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_wi.get(), wis, n * 12, hipMemcpyHostToDevice));
    HIP_TRY(launch_debug_bsdf(to_gpu_material(m), n, d_n.get<float>(), d_wo.get<float>(), d_wi.get<float>(), d_out.get<float>(), nullptr));
    HIP_TRY(hipMemcpy(out_rgb, d_out.get(), n * 12, hipMemcpyDeviceToHost));
    return RPT_OK;
}
int rpt_debug_camera_sample(const rpt_camera* cam, const rpt_render_params* prm, uint64_t seed, uint32_t sample,
                            float* origins, float* dirs, uint32_t* next_word) {
    if (!cam || !prm || !origins || !dirs) return fail(RPT_ERR_INVALID, "null argument");
    if (prm->width == 0 || prm->height == 0) return fail(RPT_ERR_INVALID, "empty frame");
    if (uint64_t(prm->width) * prm->height > (1ull << 31)) return fail(RPT_ERR_INVALID, "image too large");
    if (!launch_debug_camera_sample) return fail(RPT_ERR_UNSUPPORTED, "rpt_debug_camera_sample: built without the kernels");
    const size_t n = size_t(prm->width) * prm->height;
    rpti::DevMem d_o, d_d, d_w;
    HIP_TRY(hook_scratch(d_o, n * 12));
    HIP_TRY(hook_scratch(d_d, n * 12));
    if (next_word) HIP_TRY(hook_scratch(d_w, n * 4));
    HIP_TRY(launch_debug_camera_sample(camera_g(cam), prm->width, prm->height, inv_dim_of(prm), seed_mix(seed), sample, d_o.get<float>(),
                                       d_d.get<float>(), next_word ? d_w.get<uint32_t>() : nullptr, nullptr));
    HIP_TRY(hipMemcpy(origins, d_o.get(), n * 12, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(dirs, d_d.get(), n * 12, hipMemcpyDeviceToHost));
    if (next_word) HIP_TRY(hipMemcpy(next_word, d_w.get(), n * 4, hipMemcpyDeviceToHost));
    return RPT_OK;
}
int rpt_debug_camera_rays(const rpt_camera* cam, const rpt_render_params* prm, uint64_t seed, uint32_t sample,
                          float* origins, float* dirs) {
    return rpt_debug_camera_sample(cam, prm, seed, sample, origins, dirs, nullptr);   // (same kernel, same argument checks)
}
// The per-call hooks on a committed scene.  What the caller got wrong (null arrays, the light's kind, a scene without a medium) is
// reported before the scene's state, so those answers need no device.
int rpt_debug_light_sample(rpt_scene* s, uint32_t light, uint64_t n, const float* positions, uint64_t seed, float* v, float* nrm,
                           float* pdf, float* intensity, float* wi, float* dist, uint32_t* next_word) {
    if (!s || !positions || !v || !nrm || !pdf || !intensity || !wi || !dist || !next_word) return fail(RPT_ERR_INVALID, "null argument");
    if (rpti::light_kind(s, light) != int(L_OBJECT)) return fail(RPT_ERR_INVALID, "rpt_debug_light_sample: not a Light::Object");
    if (!s->committed) return fail(RPT_ERR_STATE, "rpt_scene_commit must be called first");
    if (s->dev.arena64) return fail(RPT_ERR_STATE, "rpt_debug_light_sample: the scene was committed with epsilon_policy = 1 (rpt_debug_light_sample_f64)");
    if (!launch_debug_light_sample) return fail(RPT_ERR_UNSUPPORTED, "rpt_debug_light_sample: built without the kernels");
    if (n == 0) return RPT_OK;
    if (n > 0xFFFFFFFFull) return fail(RPT_ERR_INVALID, "rpt_debug_light_sample: the case number keys a 32-bit stream field");
    HIP_TRY(hipSetDevice(s->device));
    if (int rc = rpti::wait_for_move(s, nullptr)) return rc;   // (the hook launches on the null stream: behind the last move of the scene's spheres)
    rpti::DevMem d_pos, d_out;   // d_out: v, nrm, intensity, wi (3 n each), pdf, dist, next_word (n each)
    HIP_TRY(hook_scratch(d_pos, n * 12));
    HIP_TRY(hook_scratch(d_out, n * 60));
    HIP_TRY(hipMemcpy(d_pos.get(), positions, n * 12, hipMemcpyHostToDevice));
    float* const o = d_out.get<float>();
    LightSampleArgs q{};
    q.light = light;
    q.n = n;
    q.seed_mixed = seed_mix(seed);
    q.pos = d_pos.get<float>();
    q.v = o; q.nrm = o + 3 * n; q.intensity = o + 6 * n; q.wi = o + 9 * n;
    q.pdf = o + 12 * n; q.dist = o + 13 * n;
    q.next_word = reinterpret_cast<uint32_t*>(o + 14 * n);
    HIP_TRY(launch_debug_light_sample(s->view, q, nullptr));
    HIP_TRY(hipMemcpy(v, q.v, n * 12, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(nrm, q.nrm, n * 12, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(intensity, q.intensity, n * 12, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(wi, q.wi, n * 12, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(pdf, q.pdf, n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(dist, q.dist, n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(next_word, q.next_word, n * 4, hipMemcpyDeviceToHost));
    return RPT_OK;
}
int rpt_debug_env_color(rpt_scene* s, uint64_t n, const float* dirs, float* rgb) {
    if (!s || !dirs || !rgb) return fail(RPT_ERR_INVALID, "null argument");
    if (!s->committed) return fail(RPT_ERR_STATE, "rpt_scene_commit must be called first");
    if (s->dev.arena64) return fail(RPT_ERR_STATE, "rpt_debug_env_color: the scene was committed with epsilon_policy = 1 (rpt_debug_env_color_f64)");
    if (!launch_debug_env_color) return fail(RPT_ERR_UNSUPPORTED, "rpt_debug_env_color: built without the kernels");
    if (n == 0) return RPT_OK;
    HIP_TRY(hipSetDevice(s->device));
    if (int rc = rpti::wait_for_move(s, nullptr)) return rc;   // (the hook launches on the null stream: behind the last move of the scene's spheres)
    rpti::DevMem d_d, d_c;
    HIP_TRY(hook_scratch(d_d, n * 12));
    HIP_TRY(hook_scratch(d_c, n * 12));
    HIP_TRY(hipMemcpy(d_d.get(), dirs, n * 12, hipMemcpyHostToDevice));
    HIP_TRY(launch_debug_env_color(s->view, n, d_d.get<float>(), d_c.get<float>(), nullptr));
    HIP_TRY(hipMemcpy(rgb, d_c.get(), n * 12, hipMemcpyDeviceToHost));
    return RPT_OK;
}
int rpt_debug_medium_distance(rpt_scene* s, uint64_t n, uint64_t seed, float* dmed, float* t_limit) {
    if (!s || !dmed || !t_limit) return fail(RPT_ERR_INVALID, "null argument");
    if (s->media.empty()) return fail(RPT_ERR_INVALID, "rpt_debug_medium_distance: the scene has no medium");
    if (!s->committed) return fail(RPT_ERR_STATE, "rpt_scene_commit must be called first");
    if (s->dev.arena64) return fail(RPT_ERR_STATE, "rpt_debug_medium_distance: the scene was committed with epsilon_policy = 1");
    if (!launch_debug_medium_distance) return fail(RPT_ERR_UNSUPPORTED, "rpt_debug_medium_distance: built without the kernels");
    if (n == 0) return RPT_OK;
    if (n > 0xFFFFFFFFull) return fail(RPT_ERR_INVALID, "rpt_debug_medium_distance: the case number keys a 32-bit stream field");
    HIP_TRY(hipSetDevice(s->device));
    if (int rc = rpti::wait_for_move(s, nullptr)) return rc;   // (the hook launches on the null stream: behind the last move of the scene's spheres)
    rpti::DevMem d_m, d_t;
    HIP_TRY(hook_scratch(d_m, n * 4));
    HIP_TRY(hook_scratch(d_t, n * 4));
    HIP_TRY(launch_debug_medium_distance(s->view, n, seed_mix(seed), d_m.get<float>(), d_t.get<float>(), nullptr));
    HIP_TRY(hipMemcpy(dmed, d_m.get(), n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(t_limit, d_t.get(), n * 4, hipMemcpyDeviceToHost));
    return RPT_OK;
}
int rpt_debug_shadow_test(rpt_scene* s, uint32_t light, uint64_t n, const float* origins, const float* dirs, const float* dist,
                          int32_t* out_flag, float* out_t) {
    if (!s || !origins || !dirs || !dist || !out_flag || !out_t) return fail(RPT_ERR_INVALID, "null argument");
    if (rpti::light_kind(s, light) != int(L_OBJECT)) return fail(RPT_ERR_INVALID, "rpt_debug_shadow_test: not a Light::Object");
    if (!s->committed) return fail(RPT_ERR_STATE, "rpt_scene_commit must be called first");
    if (s->dev.arena64) return fail(RPT_ERR_STATE, "rpt_debug_shadow_test: the scene was committed with epsilon_policy = 1");
    if (s->view.n_nodes != 0 || s->view.scene_bvh || s->view.n_inst)
        return fail(RPT_ERR_UNSUPPORTED, "rpt_debug_shadow_test: the scene has a tree (the query is the linear scan's)");
    if (!launch_debug_shadow_test) return fail(RPT_ERR_UNSUPPORTED, "rpt_debug_shadow_test: built without the kernels");
    if (n == 0) return RPT_OK;
    HIP_TRY(hipSetDevice(s->device));
    if (int rc = rpti::wait_for_move(s, nullptr)) return rc;   // (the hook launches on the null stream: behind the last move of the scene's spheres)
    rpti::DevMem d_in, d_out;   // d_in: origins, dirs (3 n each), dist (n); d_out: flag, t (n each)
    HIP_TRY(hook_scratch(d_in, n * 28));
    HIP_TRY(hook_scratch(d_out, n * 8));
    float* const in = d_in.get<float>();
    HIP_TRY(hipMemcpy(in, origins, n * 12, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(in + 3 * n, dirs, n * 12, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(in + 6 * n, dist, n * 4, hipMemcpyHostToDevice));
    ShadowTestArgs q{};
    q.light = light;
    q.n = n;
    q.o = in; q.d = in + 3 * n; q.dist = in + 6 * n;
    q.flag = d_out.get<int32_t>();
    q.t = d_out.get<float>() + n;
    HIP_TRY(launch_debug_shadow_test(s->view, q, nullptr));
    HIP_TRY(hipMemcpy(out_flag, q.flag, n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_t, q.t, n * 4, hipMemcpyDeviceToHost));
    return RPT_OK;
}
int rpt_shadow_scan_info(rpt_scene* s, uint32_t light, uint32_t out[4]) {
    if (!s || !out) return fail(RPT_ERR_INVALID, "null argument");
    if (rpti::light_kind(s, light) != int(L_OBJECT)) return fail(RPT_ERR_INVALID, "rpt_shadow_scan_info: not a Light::Object");
    if (!s->committed) return fail(RPT_ERR_STATE, "rpt_scene_commit must be called first");
    if (s->dev.arena64) return fail(RPT_ERR_STATE, "rpt_shadow_scan_info: the scene was committed with epsilon_policy = 1");
    if (light >= s->light_records.size()) return fail(RPT_ERR_STATE, "rpt_shadow_scan_info: the light was added after the commit");
    const Light& L = s->light_records[light];
    out[0] = L.twin_lo;
    out[1] = L.twin_hi;
    out[2] = (bits_u(L.color.w) != 0u && bvh_mode(s->view) == 0) ? 1u : 0u;   // (only the scan kernels read the mark)
    out[3] = uint32_t(L.twin_object);
    return RPT_OK;
}
int rpt_scan_jit_info(rpt_scene* s, int64_t out[8], char* text, uint64_t text_capacity) {
    if (!s || !out) return fail(RPT_ERR_INVALID, "null argument");
    if (!text && text_capacity) return fail(RPT_ERR_INVALID, "rpt_scan_jit_info: a capacity without a buffer");
    if (!s->committed) return fail(RPT_ERR_STATE, "rpt_scene_commit must be called first");
    const rpti::ScanJit& j = s->jit;
    std::string shape = j.shape_text, reason = j.reason;
    int state = j.state;
    if (!j.probed) {   // no render yet: the shape the first one will see
        rpti::ScanShape h;
        if (rpti::scan_shape_of(s->view, &h, &reason)) shape = rpti::scan_shape_string(h);
        else state = RPT_SCAN_JIT_OUT_OF_SCOPE;
    }
    if (s->opt.scan_jit == 0) { state = RPT_SCAN_JIT_OFF; reason = "option scan_jit = 0"; }
    out[0] = state;
    out[1] = j.cache;
    out[2] = int64_t(j.compile_ms * 1000.0);
    out[3] = j.vgprs;
    out[4] = j.scratch;
    out[5] = int64_t(j.launches);
    {
        std::lock_guard<std::mutex> lock(rpti::g_jit_mutex);
        out[6] = int64_t(rpti::g_jit_compiles);
    }
    out[7] = j.aot_vgprs;
    if (text_capacity) {
        const std::string t = shape + "\n" + reason;
        const size_t n = std::min<size_t>(t.size(), size_t(text_capacity) - 1);
        std::memcpy(text, t.data(), n);
        text[n] = 0;
    }
    return RPT_OK;
}
int rpt_scan_jit_structure(rpt_scene* s, char* text, uint64_t text_capacity) {
    if (!s || !text || !text_capacity) return fail(RPT_ERR_INVALID, "null argument");
    if (!s->committed) return fail(RPT_ERR_STATE, "rpt_scene_commit must be called first");
    std::string why;
    rpti::ScanShape h;
    const std::string t = rpti::scan_shape_of(s->view, &h, &why) ? rpti::scan_struct_string(s->jit.structure) : std::string();   // (outside the scope: empty, as the shape)
    const size_t n = std::min<size_t>(t.size(), size_t(text_capacity) - 1);
    std::memcpy(text, t.data(), n);
    text[n] = 0;
    return RPT_OK;
}
int rpt_scan_jit_forget(void) {
    std::lock_guard<std::mutex> lock(rpti::g_jit_mutex);
    const int n = int(rpti::g_jit_objects.size());
    rpti::g_jit_objects.clear();   // (loaded modules stay: scenes that run them keep their functions)
    return n;
}
int rpt_debug_distance_pair(float sigma_t, uint32_t k0, uint32_t n, float* out_new, float* out_guarded) {
    if (!out_new || !out_guarded) return fail(RPT_ERR_INVALID, "null argument");
    if (!(sigma_t > 0.f) || !(sigma_t < INFINITY)) return fail(RPT_ERR_INVALID, "rpt_debug_distance_pair: sigma_t must be positive and finite");
    if (k0 >= (1u << 23) || n > (1u << 23) - k0) return fail(RPT_ERR_INVALID, "rpt_debug_distance_pair: a draw has 23 bits (k0 + n <= 2^23)");
    if (!launch_debug_distance_pair) return fail(RPT_ERR_UNSUPPORTED, "rpt_debug_distance_pair: built without the kernels");
    if (n == 0) return RPT_OK;
    rpti::DevMem d_out;
    HIP_TRY(hook_scratch(d_out, size_t(n) * 8));
    HIP_TRY(launch_debug_distance_pair(sigma_t, k0, n, d_out.get<float>(), d_out.get<float>() + n, nullptr));
    HIP_TRY(hipMemcpy(out_new, d_out.get<float>(), size_t(n) * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_guarded, d_out.get<float>() + n, size_t(n) * 4, hipMemcpyDeviceToHost));
    return RPT_OK;
}

int rpt_debug_draw_forms(uint64_t seed, uint32_t n, uint32_t* out_new, uint32_t* out_ref) {
    if (!out_new || !out_ref) return fail(RPT_ERR_INVALID, "null argument");
    if (n > (1u << 20)) return fail(RPT_ERR_INVALID, "rpt_debug_draw_forms: at most 2^20 lanes");   // 1.15 GB per side on the device
    if (!launch_debug_draw_forms) return fail(RPT_ERR_UNSUPPORTED, "rpt_debug_draw_forms: built without the kernels");
    if (n == 0) return RPT_OK;
    const size_t bytes = size_t(n) * kDrawFormWords * 4;
    const float inv[3] = {1.f / 64.f, 1.f / 1024.f, 1.f / 3000.f};
    rpti::DevMem d_new, d_ref;
    HIP_TRY(hook_scratch(d_new, bytes));
    HIP_TRY(hook_scratch(d_ref, bytes));
    HIP_TRY(launch_debug_draw_forms(seed_mix(seed), n, inv, d_new.get<uint32_t>(), d_ref.get<uint32_t>(), nullptr));
    HIP_TRY(hipMemcpy(out_new, d_new.get(), bytes, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_ref, d_ref.get(), bytes, hipMemcpyDeviceToHost));
    return RPT_OK;
}

// stage_bounce on a material descriptor: needs no scene.  (The medium enters through its albedo and colour alone.)
int rpt_debug_bounce(const rpt_material* m, uint32_t max_bounces, uint32_t depth, int32_t in_medium, int32_t medium_event,
                     float albedo_med, const float* medium_color, uint64_t n, const float* normals, const float* rds, uint64_t seed,
                     int32_t* flag, float* wi, float* k, uint32_t* next_word) {
    std::string why;
    if (!check_material(m, why)) return fail(RPT_ERR_INVALID, why);
    if (!medium_color || !normals || !rds || !flag || !wi || !k || !next_word) return fail(RPT_ERR_INVALID, "null argument");
    if (medium_event && !in_medium) return fail(RPT_ERR_INVALID, "rpt_debug_bounce: a medium event needs in_medium");
    if (n > 0xFFFFFFFFull) return fail(RPT_ERR_INVALID, "rpt_debug_bounce: the case number keys a 32-bit stream field");
    if (!launch_debug_bounce) return fail(RPT_ERR_UNSUPPORTED, "rpt_debug_bounce: built without the kernels");
    if (n == 0) return RPT_OK;
    rpti::DevMem d_in, d_out;   // d_in: normals, rds (3 n each); d_out: wi, k (3 n each), flag, next_word (n each)
    HIP_TRY(hook_scratch(d_in, n * 24));
    HIP_TRY(hook_scratch(d_out, n * 32));
    float* const in = d_in.get<float>();
    float* const o = d_out.get<float>();
    HIP_TRY(hipMemcpy(in, normals, n * 12, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(in + 3 * n, rds, n * 12, hipMemcpyHostToDevice));
    BounceArgs q{};
    q.m = to_gpu_material(m);
    q.max_bounces = max_bounces;
    q.depth = depth;
    q.in_medium = in_medium ? 1u : 0u;
    q.medium_event = medium_event ? 1u : 0u;
    q.albedo_med = albedo_med;
    for (int i = 0; i < 3; i++) q.mcol[i] = medium_color[i];
    q.n = n;
    q.seed_mixed = seed_mix(seed);
    q.nrm = in; q.rd = in + 3 * n;
    q.wi = o; q.k = o + 3 * n;
    q.flag = reinterpret_cast<int32_t*>(o + 6 * n);
    q.next_word = reinterpret_cast<uint32_t*>(o + 7 * n);
    HIP_TRY(launch_debug_bounce(q, nullptr));
    HIP_TRY(hipMemcpy(wi, q.wi, n * 12, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(k, q.k, n * 12, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(flag, q.flag, n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(next_word, q.next_word, n * 4, hipMemcpyDeviceToHost));
    return RPT_OK;
}

}  // extern "C"

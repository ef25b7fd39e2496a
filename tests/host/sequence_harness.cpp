// Test infrastructure (see hip_stubs.h): one committed room scene driven through mixed call sequences -- sizes, shards, tile
// lists, feature passes -- on two stream handles and the null stream, with the real rpt_capi.cpp and a model of what the device
// still has in flight.  tests/test_host_call_sequences.py builds and runs it under ASan + UBSan and plain.
//
// The model.  Every stubbed launch records the memory it was handed: the tile list with a copy of its ids (compared with the
// call's own at the launch, and with the list again when the launch retires), the slab, the work counter, the frame or planes.
// A record is in flight until something orders the launch before the operation at hand:
//   * an operation on the same stream;
//   * a hipStreamWaitEvent, directly or through a chain, on an event recorded after the launch;
//   * the host having synchronised with it: hipStreamSynchronize of its stream (and of whatever that stream had waited for),
//     hipEventSynchronize, hipDeviceSynchronize, hipFree (which synchronises the device), or a blocking call on the null stream
//     for the null stream's own launches.
// The two stream handles stand for non-blocking streams (torch.cuda.Stream): a blocking hipMemcpy / hipMemset on the null stream
// orders nothing on them.  A finding is
//   * a copy or memset that writes memory a launch in flight was handed, or reads what it writes;
//   * a launch that writes memory another launch in flight reads or writes (one slab or work counter under two launches);
//   * a launch whose tile ids are not rpt_shard_tiles of the call's own parameters (the caller's list for a tile-list render), or
//     whose slab is smaller than its items need;
//   * a tile list that has changed between a launch and its retirement;
//   * a sharded render whose frame was not cleared on the launch's stream before the resolve.
// Findings are printed and make the exit code 1.  The photon camera pass lives in photon.hip and does not link here.
#include "hip_stubs.h"
#include "../../rpt_amd/csrc/rpt_capi.cpp"

#include <cstdio>
#include <map>
#include "../../include/rpt.hpp"

namespace {
using Clock = std::map<hipStream_t, uint64_t>;   // stream -> the last of its launches known to be complete
void merge(Clock& into, const Clock& from) {
    for (auto& kv : from) into[kv.first] = std::max(into[kv.first], kv.second);
}
struct Region {
    const char* name;
    const char* lo;
    size_t n;
    bool written;
};
struct Launch {
    const char* kernel;
    hipStream_t st;
    uint64_t seq;
    std::vector<Region> mem;
    int call;
    std::vector<char> ids;   // the tile list (mem[0]) as it was at the launch
};
// What the entry point under way must hand to its launches.
struct Expect {
    int call = 0;
    std::string what;
    std::vector<uint32_t> tiles;
    uint32_t width = 0, height = 0, tiles_x = 0;
    hipStream_t st = nullptr;
    const void* frame = nullptr;   // a sharded render: cleared on `st` before the resolve (device entry points: the caller's frame)
    size_t frame_bytes = 0;
    bool cleared = false;
    int launches = 0;
};

struct Model final : StubObserver {
    std::map<const char*, size_t> allocs;
    std::map<hipStream_t, uint64_t> seq;
    std::map<hipStream_t, Clock> seen;
    std::map<hipEvent_t, Clock> events;
    Clock host;
    std::vector<Launch> live;
    Expect cur;
    int findings = 0, launches = 0, copies = 0;

    void finding(const std::string& msg) {
        findings++;
        std::printf("FINDING call %d (%s): %s\n", cur.call, cur.what.c_str(), msg.c_str());
    }
    static const char* name_of(hipStream_t st) {
        return st == nullptr ? "null stream" : st == reinterpret_cast<hipStream_t>(uintptr_t(0x100)) ? "stream 1" : "stream 2";
    }
    bool ordered_before(const Launch& l, hipStream_t st) {
        if (host[l.st] >= l.seq) return true;
        if (l.st == st) return true;
        auto it = seen.find(st);
        if (it == seen.end()) return false;
        auto k = it->second.find(l.st);
        return k != it->second.end() && k->second >= l.seq;
    }
    void retire() {
        std::vector<Launch> keep;
        for (auto& l : live) {
            if (host[l.st] < l.seq) { keep.push_back(std::move(l)); continue; }
            if (!l.ids.empty() && std::memcmp(l.ids.data(), l.mem[0].lo, l.ids.size()) != 0) {
                findings++;
                std::printf("FINDING %s of call %d: its tile list changed while it was in flight\n", l.kernel, l.call);
            }
        }
        live.swap(keep);
    }
    static bool overlap(const char* a, size_t na, const char* b, size_t nb) { return na && nb && a < b + nb && b < a + na; }
    // an access to [p, p + n) by an operation on `st`
    void access(const char* what, const void* p, size_t n, bool writes, hipStream_t st) {
        const char* lo = static_cast<const char*>(p);
        for (auto& l : live) {
            if (ordered_before(l, st)) continue;
            for (auto& r : l.mem)
                if ((writes || r.written) && overlap(lo, n, r.lo, r.n)) {
                    char b[320];
                    std::snprintf(b, sizeof b, "%s on the %s %s %zu bytes of the %s of %s (call %d, %s), which is still in flight", what, name_of(st),
                                  writes ? "writes" : "reads", n, r.name, l.kernel, l.call, name_of(l.st));
                    finding(b);
                }
        }
    }
    size_t capacity_from(const void* p) {   // bytes from p to the end of its allocation (0: not device memory)
        const char* c = static_cast<const char*>(p);
        auto it = allocs.upper_bound(c);
        if (it == allocs.begin()) return 0;
        --it;
        return c < it->first + it->second ? size_t(it->first + it->second - c) : 0;
    }
    void launch(const char* kernel, hipStream_t st, std::vector<Region> mem) {
        launches++;
        cur.launches++;
        for (auto& r : mem) {
            if (!r.lo) continue;
            if (capacity_from(r.lo) < r.n) {
                char b[200];
                std::snprintf(b, sizeof b, "%s: the %s needs %zu bytes, its allocation has %zu from there", kernel, r.name, r.n, capacity_from(r.lo));
                finding(b);
            }
            access(kernel, r.lo, r.n, r.written, st);
        }
        std::vector<char> ids;   // (mem[0] is every launch's tile list)
        if (!mem.empty() && mem[0].lo && capacity_from(mem[0].lo) >= mem[0].n) ids.assign(mem[0].lo, mem[0].lo + mem[0].n);
        live.push_back(Launch{kernel, st, ++seq[st], std::move(mem), cur.call, std::move(ids)});
    }
    // the checks every render / resolve / feature launch shares
    void check_frame(const char* kernel, const uint32_t* tiles, uint32_t n_owned, uint32_t tiles_x, uint32_t width, uint32_t height, hipStream_t st) {
        char b[256];
        if (st != cur.st) { std::snprintf(b, sizeof b, "%s was launched on the %s, the call names the %s", kernel, name_of(st), name_of(cur.st)); finding(b); }
        if (width != cur.width || height != cur.height || tiles_x != cur.tiles_x) {
            std::snprintf(b, sizeof b, "%s: frame %u x %u, tiles_x %u; the call asks for %u x %u, %u", kernel, width, height, tiles_x, cur.width, cur.height, cur.tiles_x);
            finding(b);
        }
        if (n_owned != cur.tiles.size() * 1024u) {
            std::snprintf(b, sizeof b, "%s: %u pixel slots, the call owns %zu tiles", kernel, n_owned, cur.tiles.size());
            finding(b);
            return;   // (the list is not read beyond what the call owns)
        }
        if (capacity_from(tiles) < cur.tiles.size() * 4) { finding(std::string(kernel) + ": the tile list is shorter than the call's"); return; }
        for (size_t i = 0; i < cur.tiles.size(); i++)
            if (tiles[i] != cur.tiles[i]) {
                std::snprintf(b, sizeof b, "%s: tile %zu of the list is %u, the call's own list has %u", kernel, i, tiles[i], cur.tiles[i]);
                finding(b);
                return;
            }
    }
    void check_cleared(const char* kernel, const double* out) {
        if (cur.frame && !(cur.cleared && out == cur.frame)) finding(std::string(kernel) + ": the sharded frame was not cleared on the launch's stream before the resolve");
    }

    // ---- StubObserver
    void allocated(void* p, size_t n) override { allocs[static_cast<const char*>(p)] = n; }
    void freed(void* p) override {
        device_synchronized();
        allocs.erase(static_cast<const char*>(p));
    }
    void copied(const char* what, void* dst, const void* src, size_t n, hipStream_t st, bool blocking) override {
        copies++;
        access(what, dst, n, true, st);
        if (src) access(what, src, n, false, st);
        if (!src && !blocking && cur.frame && st == cur.st && dst == cur.frame && n >= cur.frame_bytes) cur.cleared = true;
        if (blocking) {   // the call returns when the null stream has run it: the host has seen what that stream had seen
            Clock c = seen[st];
            c[st] = seq[st];
            merge(host, c);
            retire();
        }
    }
    void stream_synchronized(hipStream_t st) override {
        Clock c = seen[st];
        c[st] = seq[st];
        merge(host, c);
        retire();
    }
    void device_synchronized() override {
        for (auto& kv : seq) host[kv.first] = kv.second;
        retire();
    }
    void event_recorded(hipEvent_t e, hipStream_t st) override {
        Clock c = seen[st];
        c[st] = seq[st];
        events[e] = c;
    }
    void event_waited(hipStream_t st, hipEvent_t e) override {
        auto it = events.find(e);
        if (it != events.end()) merge(seen[st], it->second);   // (an event never recorded orders nothing)
    }
    void event_synchronized(hipEvent_t e) override {
        auto it = events.find(e);
        if (it != events.end()) { merge(host, it->second); retire(); }
    }
    void event_destroyed(hipEvent_t e) override { events.erase(e); }
};
Model g_model;
}  // namespace

namespace rptg {
hipError_t launch_render(const RenderArgs& a, int, hipStream_t st) {
    g_model.check_frame("render_kernel", a.tiles, a.n_owned, a.tiles_x, a.width, a.height, st);
    g_model.launch("render_kernel", st, {{"tile list", reinterpret_cast<const char*>(a.tiles), size_t(a.n_tiles) * 4, false},
                                          {"slab", reinterpret_cast<const char*>(a.slab), size_t(a.n_items) * 16, true},
                                          {"work counter", reinterpret_cast<const char*>(a.queue), 8, true}});
    return hipSuccess;
}
hipError_t launch_resolve(const RenderArgs& a, double, double* out, hipStream_t st) {
    g_model.check_frame("resolve_kernel", a.tiles, a.n_owned, a.tiles_x, a.width, a.height, st);
    g_model.check_cleared("resolve_kernel", out);
    g_model.launch("resolve_kernel", st, {{"tile list", reinterpret_cast<const char*>(a.tiles), size_t(a.n_tiles) * 4, false},
                                           {"slab", reinterpret_cast<const char*>(a.slab), size_t(a.n_items) * 16, false},
                                           {"frame", reinterpret_cast<const char*>(out), size_t(a.width) * a.height * 24, true}});
    return hipSuccess;
}
hipError_t launch_render_f64(const rpt64::Args& q, int, hipStream_t st) {
    g_model.check_frame("render_kernel_f64", q.tiles, q.n_owned, q.tiles_x, q.width, q.height, st);
    g_model.launch("render_kernel_f64", st, {{"tile list", reinterpret_cast<const char*>(q.tiles), size_t(q.n_owned / 1024u) * 4, false},
                                              {"slab", reinterpret_cast<const char*>(q.slab), size_t(q.n_items) * 32, true},
                                              {"work counter", reinterpret_cast<const char*>(q.queue), 8, true}});
    return hipSuccess;
}
hipError_t launch_resolve_f64(const rpt64::Args& q, double, double* out, hipStream_t st) {
    g_model.check_frame("resolve_kernel_f64", q.tiles, q.n_owned, q.tiles_x, q.width, q.height, st);
    g_model.check_cleared("resolve_kernel_f64", out);
    g_model.launch("resolve_kernel_f64", st, {{"tile list", reinterpret_cast<const char*>(q.tiles), size_t(q.n_owned / 1024u) * 4, false},
                                               {"slab", reinterpret_cast<const char*>(q.slab), size_t(q.n_items) * 32, false},
                                               {"frame", reinterpret_cast<const char*>(out), size_t(q.width) * q.height * 24, true}});
    return hipSuccess;
}
hipError_t launch_features(const FeatureArgs& q, hipStream_t st) {
    g_model.check_frame("features_kernel", q.r.tiles, q.r.n_owned, q.r.tiles_x, q.r.width, q.r.height, st);
    g_model.launch("features_kernel", st, {{"tile list", reinterpret_cast<const char*>(q.r.tiles), size_t(q.r.n_tiles) * 4, false},
                                            {"feature slab", reinterpret_cast<const char*>(q.slab), size_t(q.r.n_items) * 64, true},
                                            {"feature ids", reinterpret_cast<const char*>(q.ids), size_t(q.r.n_owned) * 4, true}});
    return hipSuccess;
}
hipError_t launch_features_f64(const rpt64::FeatureArgs64& q, hipStream_t st) {
    g_model.check_frame("features_kernel_f64", q.a.tiles, q.a.n_owned, q.a.tiles_x, q.a.width, q.a.height, st);
    g_model.launch("features_kernel_f64", st, {{"tile list", reinterpret_cast<const char*>(q.a.tiles), size_t(q.a.n_owned / 1024u) * 4, false},
                                                {"feature slab", reinterpret_cast<const char*>(q.slab), size_t(q.a.n_items) * 64, true},
                                                {"feature ids", reinterpret_cast<const char*>(q.ids), size_t(q.a.n_owned) * 4, true}});
    return hipSuccess;
}
hipError_t launch_feature_resolve(const FeatureResolveArgs& r, hipStream_t st) {
    g_model.check_frame("feature_resolve_kernel", r.tiles, r.n_owned, r.tiles_x, r.width, r.height, st);
    std::vector<Region> mem = {{"tile list", reinterpret_cast<const char*>(r.tiles), size_t(r.n_owned / 1024u) * 4, false},
                               {"feature slab", reinterpret_cast<const char*>(r.slab), size_t(r.n_items) * 64, false},
                               {"feature ids", reinterpret_cast<const char*>(r.ids), size_t(r.n_owned) * 4, false}};
    for (double* plane : {r.albedo, r.normal, r.depth})
        if (plane) mem.push_back({"feature plane", reinterpret_cast<const char*>(plane), size_t(r.width) * r.height * 24, true});
    g_model.launch("feature_resolve_kernel", st, std::move(mem));
    return hipSuccess;
}
hipError_t render_occupancy(bool, int, int* b, int) { *b = 4; return hipSuccess; }
size_t stream_scratch_bytes_per_block() { return 0; }
int bvh_mode(const SceneView& sc) { return sc.scene_bvh ? 2 : (sc.n_nodes ? 1 : 0); }
hipError_t render_f64_occupancy(bool, int* blocks_per_cu) { *blocks_per_cu = 4; return hipSuccess; }
hipError_t launch_intersect(const SceneView&, uint64_t, const float*, const float*, float*, int32_t*, float*, bool, hipStream_t) { return hipSuccess; }
hipError_t launch_debug_rng(uint64_t, uint32_t, uint32_t, uint32_t, uint32_t*, hipStream_t) { return hipSuccess; }
hipError_t launch_debug_sample_f(const Material&, uint64_t, const float*, const float*, uint64_t, float*, float*, int32_t*, hipStream_t) { return hipSuccess; }
hipError_t launch_debug_bsdf(const Material&, uint64_t, const float*, const float*, const float*, float*, hipStream_t) { return hipSuccess; }
hipError_t launch_buffer_add(uint32_t, const double*, double*, double*, hipStream_t) { return hipSuccess; }
hipError_t launch_buffer_image(uint32_t, uint32_t, uint32_t, uint32_t, const double*, uint8_t*, hipStream_t) { return hipSuccess; }
hipError_t launch_buffer_variance(uint32_t, uint32_t, const double*, const double*, double*, hipStream_t) { return hipSuccess; }
}  // namespace rptg
namespace rpti { void photon_release(void*) {} }

namespace {
enum Kind { RENDER, TILES, FEATURES, HOST_RENDER };
struct Step {
    Kind kind;
    uint32_t w, h, rank, count;
};
const std::vector<uint32_t> kList = {4, 0, 8};   // what a TILES step renders
const rpt_camera kCam{{2.5, 2, -6}, {0, 0, 1}, {0, 1, 0}, 0.8, 0, 1};
hipStream_t const kS1 = reinterpret_cast<hipStream_t>(uintptr_t(0x100)), kS2 = reinterpret_cast<hipStream_t>(uintptr_t(0x200));
constexpr size_t kMaxFrame = size_t(160) * 96 * 24;

void add(rpt_scene* s, const rpt::Shape& sh, bool light = false) {
    rpt_shape_desc d = sh.desc();
    rpt_material m{};
    m.kind = RPT_MAT_LAMBERTIAN;
    m.albedo[0] = m.albedo[1] = m.albedo[2] = 0.7;
    m.emittance = light ? 10.0 : 0.0;
    if (light) { if (rpt_scene_add_light_object(s, &d, &m) != 0) std::printf("light rejected: %s\n", rpt_last_error()); }
    else if (rpt_scene_add_object(s, &d, &m) < 0) std::printf("object rejected: %s\n", rpt_last_error());
}
rpt_scene* room(int eps) {
    using namespace rpt;
    rpt_scene* s = rpt_scene_create();
    rpt_scene_set_option(s, "epsilon_policy", eps);
    add(s, polygon({{0, 0, 0}, {0, 0, 5}, {5, 0, 5}, {5, 0, 0}}));
    add(s, polygon({{0, 5, 0}, {5, 5, 0}, {5, 5, 5}, {0, 5, 5}}));
    add(s, polygon({{0, 0, 5}, {0, 5, 5}, {5, 5, 5}, {5, 0, 5}}));
    add(s, cube().scale({1, 2, 1}).rotate_y(0.3).translate({3.5, 1, 3.5}));
    add(s, sphere().translate({2, 1, 2}));
    add(s, polygon({{2, 4.9, 2}, {3, 4.9, 2}, {3, 4.9, 3}, {2, 4.9, 3}}), true);
    const int rc = rpt_scene_commit(s, 0);
    if (rc) std::printf("commit failed: %d %s\n", rc, rpt_last_error());
    return s;
}
struct Driver {
    rpt_scene* s;
    std::vector<void*> frames;     // one device frame per call of a sequence: no two calls of it share an output
    std::vector<double> host_frame;
    void* d_list = nullptr;
    size_t next_frame = 0;
    explicit Driver(rpt_scene* scene) : s(scene), host_frame(kMaxFrame / 8) {
        for (int i = 0; i < 24; i++) {   // (the longest sequence has 20 calls)
            void* p = nullptr;
            (void)hipMalloc(&p, kMaxFrame * 3);
            frames.push_back(p);
        }
        (void)hipMalloc(&d_list, kList.size() * 4);   // the caller's tile list: uploaded once, before anything reads it
        (void)hipMemcpy(d_list, kList.data(), kList.size() * 4, hipMemcpyHostToDevice);
    }
    ~Driver() {
        for (void* p : frames) (void)hipFree(p);
        (void)hipFree(d_list);
    }
    int call(const Step& st, hipStream_t stream) {
        Expect e;
        e.call = g_model.cur.call + 1;
        e.width = st.w; e.height = st.h; e.tiles_x = (st.w + 31) / 32;
        e.st = st.kind == HOST_RENDER ? nullptr : stream;
        char what[96];
        static const char* const names[] = {"rpt_render_sample_device", "rpt_render_sample_tiles_device", "rpt_render_features_device", "rpt_render_sample"};
        std::snprintf(what, sizeof what, "%s %u x %u shard %u/%u on the %s", names[st.kind], st.w, st.h, st.rank, st.count, Model::name_of(e.st));
        e.what = what;
        if (st.kind == TILES) e.tiles = kList;
        else {
            e.tiles.resize(size_t(e.tiles_x) * ((st.h + 31) / 32));
            e.tiles.resize(size_t(rpt_shard_tiles(st.w, st.h, st.rank, st.count, e.tiles.data(), e.tiles.size())));
        }
        void* frame = frames[next_frame++ % frames.size()];
        if (st.count > 1 && st.kind == RENDER) { e.frame = frame; e.frame_bytes = size_t(st.w) * st.h * 24; }
        g_model.cur = e;
        const rpt_render_params prm{st.w, st.h, 0.0, 3, st.rank, st.count};
        const uint32_t spp = 8, offset = 0;
        int rc = 0;
        switch (st.kind) {
        case RENDER: rc = rpt_render_sample_device(s, &kCam, &prm, spp, 7, offset, frame, stream); break;
        case TILES: rc = rpt_render_sample_tiles_device(s, &kCam, &prm, spp, 7, offset, d_list, uint32_t(kList.size()), frame, stream); break;
        case FEATURES: {
            char* p = static_cast<char*>(frame);
            rc = rpt_render_features_device(s, &kCam, &prm, spp, 7, offset, p, p + kMaxFrame, p + 2 * kMaxFrame, stream);
            break;
        }
        case HOST_RENDER: rc = rpt_render_sample(s, &kCam, &prm, spp, 7, offset, host_frame.data()); break;
        }
        if (rc) g_model.finding(std::string("the call failed: ") + rpt_last_error());
        else if (g_model.cur.launches == 0) g_model.finding("the call launched nothing");
        return rc;
    }
};
std::vector<Step> sizes() { return {{RENDER, 96, 96, 0, 1}, {RENDER, 96, 32, 0, 1}, {RENDER, 33, 17, 0, 1}, {RENDER, 96, 96, 0, 1}, {RENDER, 160, 96, 0, 1}}; }
std::vector<Step> shards() { return {{RENDER, 96, 96, 0, 2}, {RENDER, 96, 96, 1, 2}, {RENDER, 96, 96, 0, 1}}; }
std::vector<Step> tile_list() { return {{RENDER, 96, 96, 0, 1}, {TILES, 96, 96, 0, 1}, {RENDER, 96, 32, 0, 1}, {RENDER, 96, 96, 0, 1}}; }
std::vector<Step> features() { return {{RENDER, 96, 96, 0, 1}, {FEATURES, 96, 32, 0, 1}, {RENDER, 33, 17, 0, 1}, {FEATURES, 96, 96, 0, 2}, {RENDER, 96, 96, 1, 2}}; }
std::vector<Step> many_frames() {   // more frames than a scene keeps lists for, then the first again
    std::vector<Step> steps;
    for (uint32_t k = 1; k <= 18; k++) steps.push_back({RENDER, 8 + 8 * k, 16 + (k & 1), 0, 1});
    steps.push_back(steps[0]);
    steps.push_back(steps[17]);
    return steps;
}
}  // namespace

int main() {
    g_stub_observer = &g_model;
    for (int eps = 0; eps < 2; eps++) {
        rpt_scene* s = room(eps);
        {
            Driver d(s);
            struct Named { const char* name; std::vector<Step> steps; };
            const Named groups[] = {{"sizes", sizes()}, {"shards", shards()}, {"tile list", tile_list()}, {"features", features()},
                                    {"many frames", many_frames()}};
            for (const Named& g : groups)
                for (int policy = 0; policy < 3; policy++) {   // one stream; two streams in turn; every other call through the host entry point
                    const int before = g_model.findings, launches = g_model.launches;
                    for (size_t i = 0; i < g.steps.size(); i++) {
                        Step st = g.steps[i];
                        hipStream_t stream = policy == 1 && (i & 1) ? kS2 : kS1;
                        if (policy == 2 && (i & 1) && st.kind == RENDER) st.kind = HOST_RENDER;
                        d.call(st, stream);
                    }
                    (void)hipDeviceSynchronize();
                    static const char* const policies[] = {"one stream", "two streams in turn", "a stream and the host entry point in turn"};
                    std::printf("%s %s, %s: %d launches, %d findings\n", eps ? "epsilon" : "fp32", g.name, policies[policy], g_model.launches - launches,
                                g_model.findings - before);
                }
        }
        rpt_scene_destroy(s);
    }
    std::printf("launches=%d copies=%d findings=%d still in flight=%zu\n", g_model.launches, g_model.copies, g_model.findings, g_model.live.size());
    g_stub_observer = nullptr;
    return g_model.findings ? 1 : 0;
}

// Test infrastructure for tests/test_host_temporal_clip.py: the host half of RPT_TEMPORAL_CLIP and rpt_temporal_set_clip in the real
// rpt_capi.cpp over malloc-backed HIP stubs (hip_stubs.h; flatten_harness.cpp's launcher stubs are reused), run as a program of its
// own under AddressSanitizer + UBSan and plain.  The stub of the accumulation kernel reads every byte of its input planes and records
// its arguments; main() checks the refusals of rpt_temporal_set_clip in their order and before the handle, that the setter touches no
// device, the defaults when it was never called, that the three values and the flag arrive in TemporalArgs through all three entry
// points and only with the flag, that they persist over calls and over rpt_temporal_reset, that a refused set leaves the settings and
// a refused call launches nothing, and that the record swap and the event waits stay as temporal_harness.cpp observes them.  Prints one
// line per check; exit code 1 on a failure.
#define main flatten_harness_main
#include "flatten_harness.cpp"
#undef main

#include <cmath>
#include <vector>

namespace {
struct Seen {
    rptg::TemporalArgs a;
    hipStream_t st;
};
std::vector<Seen> g_seen;
int g_waits = 0, g_records = 0, g_failures = 0, g_device_calls = 0;
struct Watch : StubObserver {
    void allocated(void*, size_t) override { g_device_calls++; }
    void freed(void*) override { g_device_calls++; }
    void copied(const char*, void*, const void*, size_t, hipStream_t, bool) override { g_device_calls++; }
    void stream_synchronized(hipStream_t) override { g_device_calls++; }
    void device_synchronized() override { g_device_calls++; }
    void event_recorded(hipEvent_t, hipStream_t) override { g_records++; g_device_calls++; }
    void event_waited(hipStream_t, hipEvent_t) override { g_waits++; g_device_calls++; }
    void event_synchronized(hipEvent_t) override { g_device_calls++; }
    void event_destroyed(hipEvent_t) override {}
};
double sum(const double* p, size_t n) {
    double s = 0;
    for (size_t i = 0; i < n; i++) s += p[i];
    return s;
}
void expect(bool ok, const char* what) {
    std::printf("%s: %s\n", what, ok ? "ok" : "FAILED");
    if (!ok) g_failures++;
}
bool said(const char* word) { return std::string(rpt_last_error()).find(word) != std::string::npos; }
bool clip_is(const rptg::TemporalArgs& a, uint32_t flags, uint32_t radius, double gamma, uint32_t history) {
    return a.flags == flags && a.clip_radius == radius && a.clip_gamma == gamma && a.clip_history == history;
}
}  // namespace

namespace rptg {
hipError_t launch_temporal_accumulate(const TemporalArgs& a, hipStream_t st) {
    const size_t n = size_t(a.width) * a.height;
    volatile double sink = sum(a.rgb, 3 * n) + sum(a.depth, 3 * n) + sum(a.hist_in, n * kTemporalRecDoubles);
    if (a.var) sink = sink + sum(a.var, n);
    if (a.normal) sink = sink + sum(a.normal, 3 * n);
    (void)sink;
    g_seen.push_back({a, st});
    for (size_t i = 0; i < 3 * n; i++) a.out_rgb[i] = a.rgb[i] + 1.0;
    for (size_t i = 0; i < n; i++) {
        if (a.out_var) a.out_var[i] = 2.0;
        if (a.out_len) a.out_len[i] = 3.0;
    }
    for (size_t i = 0; i < n * kTemporalRecDoubles; i++) a.hist_out[i] = 4.0;
    return hipSuccess;
}
hipError_t launch_temporal_motion_upload(void* d_table, const double* records, size_t bytes, hipStream_t) {
    g_device_calls++;
    std::memcpy(d_table, records, bytes);
    return hipSuccess;
}
hipError_t launch_buffer_mean(uint32_t n_pixels, uint32_t, const double*, const double*, double* rgb, double* var, hipStream_t) {
    for (size_t i = 0; i < 3 * size_t(n_pixels); i++) rgb[i] = 0.25;
    if (var)
        for (size_t i = 0; i < n_pixels; i++) var[i] = 0.5;
    return hipSuccess;
}
hipError_t launch_color_bytes(uint64_t n_values, const double* rgb, uint8_t* out, hipStream_t) {
    for (uint64_t i = 0; i < n_values; i++) out[i] = uint8_t(rgb[i] * 100.0);
    return hipSuccess;
}
}  // namespace rptg

int main() {
    Watch watch;
    g_stub_observer = &watch;
    const uint32_t w = 7, h = 5;
    const size_t n = size_t(w) * h;
    hipStream_t const s1 = reinterpret_cast<hipStream_t>(uintptr_t(0x100)), s2 = reinterpret_cast<hipStream_t>(uintptr_t(0x200));
    const uint32_t both = RPT_TEMPORAL_MATCH_ID | RPT_TEMPORAL_CLIP;
    const rpt_temporal_params plain{16, RPT_TEMPORAL_MATCH_ID, 0.1, 0.5}, clip{16, both, 0.1, 0.5}, clip_alone{4, RPT_TEMPORAL_CLIP, 0.0, 0.5};
    rpt_camera cams[2] = {{{0, 0, 10}, {0, 0, -1}, {0, 1, 0}, 0.5, 0, 0}, {{1, 0, 10}, {0, 0, -1}, {0, 1, 0}, 0.5, 0, 0}};
    std::vector<double> rgb(3 * n, 1.0), var(n, 0.1), normal(3 * n, 0.0), depth(3 * n, 1.0), out(3 * n), out_var(n), out_len(n);
    rpt_temporal* t = rpt_temporal_create(0, w, h);
    auto call = [&](const rpt_temporal_params& prm, int cam, hipStream_t st) {
        return rpt_temporal_accumulate_device(t, &prm, &cams[cam], rgb.data(), var.data(), normal.data(), depth.data(), out.data(), out_var.data(),
                                              out_len.data(), st);
    };
    static_assert(sizeof(rpt_temporal_params) == 24 && RPT_TEMPORAL_CLIP == 2u, "the parameters keep their size; the flag is bit 1");

    // ---- the defaults, before any set
    expect(call(clip, 0, s1) == RPT_OK && g_seen.size() == 1 && clip_is(g_seen.back().a, both, 1, 0.5, 1), "the flag with set_clip never called uses (1, 0.5, 1)");
    expect(call(plain, 1, s2) == RPT_OK && clip_is(g_seen.back().a, RPT_TEMPORAL_MATCH_ID, 0, 0.0, 0), "without the flag the three fields are zero");

    // ---- refusals, in order, all before any device call; a refused set leaves the settings
    {
        const int before = g_device_calls;
        bool ok = true;
        for (uint32_t r : {0u, 4u, 0xFFFFFFFFu}) ok = ok && rpt_temporal_set_clip(t, r, NAN, 9999) == RPT_ERR_INVALID && said("radius");
        for (double g : {double(NAN), double(INFINITY), -double(INFINITY), -1e-300, -2.0})
            ok = ok && rpt_temporal_set_clip(t, 3, g, 9999) == RPT_ERR_INVALID && said("gamma");
        for (uint32_t k : {4097u, 0xFFFFFFFFu}) ok = ok && rpt_temporal_set_clip(t, 3, 0.0, k) == RPT_ERR_INVALID && said("clip_history");
        ok = ok && rpt_temporal_set_clip(nullptr, 0, 0.5, 1) == RPT_ERR_INVALID && said("radius");
        ok = ok && rpt_temporal_set_clip(nullptr, 2, 0.5, 1) == RPT_ERR_INVALID && said("null accumulator");
        expect(ok && g_device_calls == before, "radius, gamma, clip_history and a null handle are refused in this order, before any device call");
        expect(call(clip, 0, s1) == RPT_OK && clip_is(g_seen.back().a, both, 1, 0.5, 1), "a refused set leaves the settings");
    }

    // ---- the three values and the flag arrive; the ends of every range are accepted; the setter touches no device
    {
        const int before = g_device_calls;
        bool ok = rpt_temporal_set_clip(t, 3, 1.5, 5) == RPT_OK && g_device_calls == before;
        ok = ok && call(clip, 1, s2) == RPT_OK && clip_is(g_seen.back().a, both, 3, 1.5, 5);
        expect(ok, "the three values and the flag arrive in the kernel's arguments; the setter touches no device");
        ok = call(clip_alone, 0, s1) == RPT_OK && clip_is(g_seen.back().a, RPT_TEMPORAL_CLIP, 3, 1.5, 5) && g_seen.back().a.max_history == 4;
        expect(ok, "the flag alone, without MATCH_ID, and the settings persist over calls");
        ok = call(plain, 1, s1) == RPT_OK && clip_is(g_seen.back().a, RPT_TEMPORAL_MATCH_ID, 0, 0.0, 0) && call(clip, 0, s1) == RPT_OK &&
             clip_is(g_seen.back().a, both, 3, 1.5, 5);
        expect(ok, "a call without the flag ignores them and does not forget them");
        ok = rpt_temporal_set_clip(t, 1, 0.0, 0) == RPT_OK && call(clip, 1, s1) == RPT_OK && clip_is(g_seen.back().a, both, 1, 0.0, 0);
        ok = ok && rpt_temporal_set_clip(t, 3, 1e300, 4096) == RPT_OK && call(clip, 0, s1) == RPT_OK && clip_is(g_seen.back().a, both, 3, 1e300, 4096);
        expect(ok, "the ends of the three ranges are accepted");
    }

    // ---- persistence over reset (a setting, not data)
    {
        uint32_t frames = 9;
        bool ok = rpt_temporal_set_clip(t, 2, 0.25, 3) == RPT_OK && rpt_temporal_reset(t) == RPT_OK && call(clip, 0, s2) == RPT_OK &&
                  rpt_temporal_frames(t, &frames) == RPT_OK;
        expect(ok && frames == 1 && g_seen.back().a.have_history == 0 && clip_is(g_seen.back().a, both, 2, 0.25, 3), "the settings persist over a reset");
    }

    // ---- a refused call launches nothing; the flag check admits exactly the two flags
    {
        const size_t launches = g_seen.size();
        const int before = g_device_calls;
        bool ok = true;
        for (uint32_t f : {4u, 4u | both, 0x80000000u, 8u | RPT_TEMPORAL_CLIP}) {
            const rpt_temporal_params bad{16, f, 0.1, 0.5};
            ok = ok && call(bad, 0, s1) == RPT_ERR_INVALID && said("unknown temporal flag");
        }
        rpt_temporal_params bad = clip;
        bad.max_history = 0;
        ok = ok && call(bad, 0, s1) == RPT_ERR_INVALID;
        ok = ok && rpt_temporal_accumulate_device(t, &clip, &cams[0], rgb.data(), nullptr, nullptr, depth.data(), out.data(), nullptr, nullptr, s1) == RPT_ERR_INVALID;
        ok = ok && rpt_temporal_accumulate_device(nullptr, &clip, &cams[0], rgb.data(), nullptr, normal.data(), depth.data(), out.data(), nullptr, nullptr, s1) == RPT_ERR_INVALID;
        expect(ok && g_seen.size() == launches && g_device_calls == before, "a refused call with the flag launches nothing and reaches no device");
        expect(call(clip, 1, s1) == RPT_OK && clip_is(g_seen.back().a, both, 2, 0.25, 3), "and the next call still finds the settings");
    }

    // ---- the host entry point and the frame image pass them through; a motion table rides along
    {
        const std::vector<double> table(2 * RPT_TEMPORAL_MOTION_DOUBLES, 1.0);
        bool ok = rpt_temporal_set_motion(t, table.data(), 2) == RPT_OK &&
                  rpt_temporal_accumulate(t, &clip, &cams[0], rgb.data(), var.data(), normal.data(), depth.data(), out.data(), out_var.data(), out_len.data()) == RPT_OK;
        expect(ok && clip_is(g_seen.back().a, both, 2, 0.25, 3) && g_seen.back().a.rgb != rgb.data() && g_seen.back().a.n_motion == 2 && out[0] == 2.0,
               "the host entry point passes the settings through, with a motion table");
        rpt_buffer* b = rpt_buffer_create(0, w, h, 0);
        std::vector<uint8_t> img(3 * n, 0);
        rpt_buffer_add_samples(b, rgb.data());
        rpt_buffer_add_samples(b, rgb.data());
        ok = rpt_temporal_frame_image(t, &clip, &cams[1], b, nullptr, nullptr, nullptr, normal.data(), depth.data(), img.data()) == RPT_OK;
        expect(ok && clip_is(g_seen.back().a, both, 2, 0.25, 3) && g_seen.back().a.motion == nullptr && img[0] == 125, "the frame image passes them through");
        ok = rpt_temporal_frame_image(t, &plain, &cams[1], b, nullptr, nullptr, nullptr, normal.data(), depth.data(), img.data()) == RPT_OK;
        expect(ok && clip_is(g_seen.back().a, RPT_TEMPORAL_MATCH_ID, 0, 0.0, 0), "and without the flag it passes zeros");
        rpt_buffer_destroy(b);
    }

    // ---- a second accumulator has its own settings
    {
        rpt_temporal* u = rpt_temporal_create(0, w, h);
        bool ok = rpt_temporal_set_clip(u, 3, 2.0, 7) == RPT_OK &&
                  rpt_temporal_accumulate_device(u, &clip, &cams[0], rgb.data(), var.data(), normal.data(), depth.data(), out.data(), nullptr, nullptr, s2) == RPT_OK;
        ok = ok && clip_is(g_seen.back().a, both, 3, 2.0, 7) && call(clip, 0, s1) == RPT_OK && clip_is(g_seen.back().a, both, 2, 0.25, 3);
        expect(ok, "two accumulators keep their own settings");
        g_seen.erase(g_seen.end() - 2);                                      // (u's launch: not part of t's swap chain below)
        rpt_temporal_destroy(u);
    }

    // ---- record swap and event waits, as temporal_harness.cpp observes them
    {
        bool swap = true;
        for (size_t k = 1; k < g_seen.size(); k++)
            swap = swap && g_seen[k].a.hist_in == g_seen[k - 1].a.hist_out && g_seen[k].a.hist_out == g_seen[k - 1].a.hist_in && g_seen[k].a.hist_in != g_seen[k].a.hist_out;
        expect(swap, "the two record arrays swap per call, with the flag or without");
    }
    rpt_temporal_destroy(t);
    g_stub_observer = nullptr;
    std::printf("launches=%zu waits=%d records=%d failures=%d\n", g_seen.size(), g_waits, g_records, g_failures);
    return g_failures ? 1 : 0;
}

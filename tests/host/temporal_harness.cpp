// Test infrastructure for tests/test_host_temporal.py: the host half of rpt_temporal_* in the real rpt_capi.cpp over malloc-backed
// HIP stubs (hip_stubs.h; flatten_harness.cpp's launcher stubs are reused), run as a program of its own under AddressSanitizer +
// UBSan and plain.  The stub of the accumulation kernel reads and writes every byte the kernel would (all planes, one whole record
// array each way), so an array that is too small or freed is a sanitizer report; it records its arguments, and main() checks the
// handle's life cycle, the swap of the two record arrays, the camera record stored with the history, the event that orders the
// calls of one accumulator, the check order and the host entry points' copies.  Prints one line per check; exit code 1 on a failure.
#define main flatten_harness_main
#include "flatten_harness.cpp"
#undef main

#include <vector>

namespace {
struct Seen {
    rptg::TemporalArgs a;
    hipStream_t st;
};
std::vector<Seen> g_seen;
int g_waits = 0, g_records = 0, g_failures = 0;
struct Watch : StubObserver {
    void allocated(void*, size_t) override {}
    void freed(void*) override {}
    void copied(const char*, void*, const void*, size_t, hipStream_t, bool) override {}
    void stream_synchronized(hipStream_t) override {}
    void device_synchronized() override {}
    void event_recorded(hipEvent_t, hipStream_t) override { g_records++; }
    void event_waited(hipStream_t, hipEvent_t) override { g_waits++; }
    void event_synchronized(hipEvent_t) override {}
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
}  // namespace

namespace rptg {
// Touches what temporal_accumulate_kernel touches; out = rgb + 1, the variance and the length planes 2 and 3, the new records 4.
hipError_t launch_temporal_accumulate(const TemporalArgs& a, hipStream_t st) {
    g_seen.push_back({a, st});
    const size_t n = size_t(a.width) * a.height;
    volatile double sink = sum(a.rgb, 3 * n) + sum(a.depth, 3 * n) + sum(a.hist_in, n * kTemporalRecDoubles);
    if (a.var) sink = sink + sum(a.var, n);
    if (a.normal) sink = sink + sum(a.normal, 3 * n);
    (void)sink;
    for (size_t i = 0; i < 3 * n; i++) a.out_rgb[i] = a.rgb[i] + 1.0;
    for (size_t i = 0; i < n; i++) {
        if (a.out_var) a.out_var[i] = 2.0;
        if (a.out_len) a.out_len[i] = 3.0;
    }
    for (size_t i = 0; i < n * kTemporalRecDoubles; i++) a.hist_out[i] = 4.0;
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
    const rpt_temporal_params prm{16, RPT_TEMPORAL_MATCH_ID, 0.1, 0.5};
    rpt_camera cams[3] = {{{0, 0, 10}, {0, 0, -1}, {0, 1, 0}, 0.5, 0, 0}, {{1, 0, 10}, {0, 0, -1}, {0, 1, 0}, 0.5, 0, 0}, {{2, 0, 10}, {0, 0, -1}, {0, 1, 0}, 0.6, 0, 0}};
    // exact sizes on the heap: a read or a write past a plane is a sanitizer report
    std::vector<double> rgb(3 * n, 1.0), var(n, 0.1), normal(3 * n, 0.0), depth(3 * n, 1.0), out(3 * n), out_var(n), out_len(n);

    // ---- life cycle and bad sizes
    expect(rpt_temporal_create(0, 0, 5) == nullptr && rpt_temporal_create(0, 1u << 16, 1u << 15) == nullptr, "create refuses bad sizes");
    expect(rpt_temporal_create(3, 4, 4) == nullptr, "create refuses a device that is not there");
    g_stub_malloc_limit = 100;
    expect(rpt_temporal_create(0, w, h) == nullptr, "create survives a failed allocation");
    g_stub_malloc_limit = SIZE_MAX;
    rpt_temporal_destroy(nullptr);
    rpt_temporal* t = rpt_temporal_create(0, w, h);
    uint32_t frames = 99;
    expect(t && rpt_temporal_frames(t, &frames) == RPT_OK && frames == 0, "a new accumulator holds no frame");

    // ---- check order: parameters, camera and planes before the handle; a refused call launches nothing and keeps the history
    rpt_temporal_params bad = prm;
    bad.max_history = 0;
    expect(rpt_temporal_accumulate_device(nullptr, &bad, &cams[0], rgb.data(), nullptr, normal.data(), depth.data(), out.data(), nullptr, nullptr, s1) ==
                   RPT_ERR_INVALID && std::string(rpt_last_error()).find("max_history") != std::string::npos,
           "the parameters are checked before the handle");
    expect(rpt_temporal_accumulate_device(t, &prm, &cams[0], rgb.data(), nullptr, nullptr, depth.data(), out.data(), nullptr, nullptr, s1) == RPT_ERR_INVALID &&
                   rpt_temporal_accumulate_device(t, &prm, &cams[0], rgb.data(), nullptr, normal.data(), depth.data(), rgb.data(), nullptr, nullptr, s1) ==
                           RPT_ERR_INVALID && g_seen.empty() && g_waits == 0 && g_records == 0,
           "a refused call reaches no device call");

    // ---- three calls on alternating streams: the arrays swap, the camera record travels with the history, the calls are ordered
    hipStream_t const streams[3] = {s1, s2, s1};
    bool ok = true;
    for (int k = 0; k < 3; k++)
        ok = ok && rpt_temporal_accumulate_device(t, &prm, &cams[k], rgb.data(), var.data(), normal.data(), depth.data(), out.data(), out_var.data(),
                                                  out_len.data(), streams[k]) == RPT_OK;
    expect(ok && g_seen.size() == 3, "three calls, three launches");
    if (g_seen.size() == 3) {
        const auto& a0 = g_seen[0].a;
        const auto& a1 = g_seen[1].a;
        const auto& a2 = g_seen[2].a;
        expect(a0.have_history == 0 && a1.have_history == 1 && a2.have_history == 1, "history from the second call on");
        expect(a0.hist_in != a0.hist_out && a1.hist_in == a0.hist_out && a1.hist_out == a0.hist_in && a2.hist_in == a1.hist_out && a2.hist_out == a1.hist_in,
               "the two record arrays swap per call");
        double rec[13];
        rpt_temporal_camera_record(&cams[1], rec);
        expect(std::memcmp(&a1.prev, &a0.cur, sizeof a0.cur) == 0 && std::memcmp(&a2.prev, &a1.cur, sizeof a1.cur) == 0 &&
                       std::memcmp(&a1.cur, rec, sizeof rec) == 0 && a2.cur.eye[0] == 2.0 && a2.prev.eye[0] == 1.0,
               "the camera record of a call is stored with its history");
        expect(g_seen[0].st == s1 && g_seen[1].st == s2 && g_seen[2].st == s1 && g_waits == 2 && g_records == 3,
               "every call but the first waits for its predecessor's event, whatever its stream");
        expect(a0.width == w && a0.height == h && a0.max_history == 16 && a0.flags == RPT_TEMPORAL_MATCH_ID && a0.depth_tol == 0.1 && a0.normal_tol == 0.5 &&
                       a0.rgb == rgb.data() && a0.var == var.data() && a0.normal == normal.data() && a0.depth == depth.data() && a0.out_rgb == out.data() &&
                       a0.out_var == out_var.data() && a0.out_len == out_len.data(),
               "the launch gets the call's arguments");
    }
    expect(rpt_temporal_frames(t, &frames) == RPT_OK && frames == 3, "three frames");

    // ---- reset
    expect(rpt_temporal_reset(t) == RPT_OK && rpt_temporal_frames(t, &frames) == RPT_OK && frames == 0, "reset forgets the frames");
    ok = rpt_temporal_accumulate_device(t, &prm, &cams[0], rgb.data(), nullptr, normal.data(), depth.data(), out.data(), nullptr, nullptr, nullptr) == RPT_OK;
    expect(ok && g_seen.size() == 4 && g_seen[3].a.have_history == 0 && g_seen[3].a.var == nullptr && g_seen[3].a.out_var == nullptr &&
                   g_seen[3].a.out_len == nullptr && g_waits == 3,
           "the call after a reset looks nothing up, and is still ordered behind the last one");

    // ---- the host entry point: planes up, outputs down, the optional ones only where given
    std::fill(out.begin(), out.end(), -1.0);
    std::fill(out_var.begin(), out_var.end(), -1.0);
    std::fill(out_len.begin(), out_len.end(), -1.0);
    ok = rpt_temporal_accumulate(t, &prm, &cams[1], rgb.data(), var.data(), normal.data(), depth.data(), out.data(), out_var.data(), out_len.data()) == RPT_OK;
    expect(ok && sum(out.data(), 3 * n) == 2.0 * 3 * n && sum(out_var.data(), n) == 2.0 * n && sum(out_len.data(), n) == 3.0 * n &&
                   g_seen.back().a.have_history == 1 && g_seen.back().a.rgb != rgb.data(),
           "the host entry point copies the planes up and all three outputs down");
    std::fill(out_var.begin(), out_var.end(), -1.0);
    const rpt_temporal_params no_normal{4, 0, 0.0, 0.0};
    ok = rpt_temporal_accumulate(t, &no_normal, &cams[2], rgb.data(), nullptr, nullptr, depth.data(), out.data(), nullptr, nullptr) == RPT_OK;
    expect(ok && sum(out_var.data(), n) == -1.0 * n && g_seen.back().a.var == nullptr && g_seen.back().a.normal == nullptr &&
                   g_seen.back().a.out_var == nullptr && g_seen.back().a.out_len == nullptr && g_seen.back().a.max_history == 4,
           "NULL planes and outputs stay NULL");

    // ---- rpt_temporal_frame_image: a buffer of two batches -> bytes; sizes, state and the denoiser's checks
    rpt_buffer* b = rpt_buffer_create(0, w, h, 0);
    std::vector<uint8_t> img(3 * n, 0);
    expect(rpt_temporal_frame_image(t, &prm, &cams[0], b, nullptr, nullptr, nullptr, normal.data(), depth.data(), img.data()) == RPT_ERR_STATE,
           "fewer than two batches: RPT_ERR_STATE");
    rpt_buffer_add_samples(b, rgb.data());
    rpt_buffer_add_samples(b, rgb.data());
    const size_t before = g_seen.size();
    ok = rpt_temporal_frame_image(t, &prm, &cams[0], b, nullptr, nullptr, nullptr, normal.data(), depth.data(), img.data()) == RPT_OK;
    expect(ok && g_seen.size() == before + 1 && g_seen.back().a.normal == normal.data() && g_seen.back().a.out_var != nullptr && img[0] == 125 &&
                   img[3 * n - 1] == 125,
           "frame image: mean 0.25 -> accumulate (+1) -> bytes");
    ok = rpt_temporal_frame_image(t, &no_normal, &cams[0], b, nullptr, nullptr, nullptr, normal.data(), depth.data(), img.data()) == RPT_OK;
    expect(ok && g_seen.back().a.normal == nullptr, "with normal_tol == 0 the accumulation is not handed the normal plane");
    rpt_temporal* small = rpt_temporal_create(0, 3, 3);
    rpt_denoiser* den = rpt_denoiser_create(0, 3, 3);
    const rpt_denoise_params dprm{4, RPT_DENOISE_MATCH_ID, 0.0, 0.5, 0.0};
    expect(rpt_temporal_frame_image(small, &prm, &cams[0], b, nullptr, nullptr, nullptr, normal.data(), depth.data(), img.data()) == RPT_ERR_INVALID &&
                   rpt_temporal_frame_image(t, &prm, &cams[0], b, den, &dprm, nullptr, normal.data(), depth.data(), img.data()) == RPT_ERR_INVALID &&
                   std::string(rpt_last_error()).find("sizes") != std::string::npos,
           "accumulator, buffer and denoiser must have one size");
    expect(rpt_temporal_frame_image(t, &prm, &cams[0], b, den, nullptr, nullptr, normal.data(), depth.data(), img.data()) == RPT_ERR_INVALID &&
                   rpt_temporal_frame_image(t, &prm, &cams[0], nullptr, nullptr, nullptr, nullptr, normal.data(), depth.data(), img.data()) == RPT_ERR_INVALID,
           "a denoiser needs its parameters, and the buffer must be there");
    rpt_temporal_frames(small, &frames);
    expect(frames == 0 && g_seen.size() == before + 2, "refused frame images launch nothing");

    rpt_denoiser_destroy(den);
    rpt_temporal_destroy(small);
    rpt_buffer_destroy(b);
    rpt_temporal_destroy(t);
    g_stub_observer = nullptr;
    std::printf("launches=%zu waits=%d records=%d failures=%d\n", g_seen.size(), g_waits, g_records, g_failures);
    return g_failures ? 1 : 0;
}

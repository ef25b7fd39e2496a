// Test infrastructure for tests/test_host_temporal_motion.py: the host half of rpt_temporal_set_motion* in the real rpt_capi.cpp over
// malloc-backed HIP stubs (hip_stubs.h; flatten_harness.cpp's launcher stubs are reused), run as a program of its own under
// AddressSanitizer + UBSan and plain.  The stub of the accumulation kernel reads every byte of the motion table it is given (and what
// temporal_harness.cpp's stub touches), so a table that is too small, freed or stale is a sanitizer report; it records its arguments
// and the table's first double, and main() checks that a table reaches the next launch and no later one, that a refused call leaves
// it and a reset drops it, that a second set replaces the first and NULL / 0 clears, that a value that is not finite is refused before
// any device call, that a growing table reallocates without a leak, that the device variant passes the caller's pointer through,
// and that the record swap and the event waits stay as temporal_harness.cpp observes them.  Prints one line per check; exit code 1 on
// a failure.
#define main flatten_harness_main
#include "flatten_harness.cpp"
#undef main

#include <cmath>
#include <vector>

namespace {
struct Seen {
    rptg::TemporalArgs a;
    hipStream_t st;
    double first;       // table[0] at launch time, or 0
    double total;       // the sum of every double of the table
    int waits_before;   // event waits seen when the kernel was launched
};
struct Upload {
    void* dst;
    const double* src;
    size_t bytes;
    hipStream_t st;
    int waits_before;
};
std::vector<Seen> g_seen;
std::vector<Upload> g_uploads;
int g_waits = 0, g_records = 0, g_failures = 0, g_allocs = 0, g_frees = 0, g_device_calls = 0;
struct Watch : StubObserver {
    void allocated(void*, size_t) override { g_allocs++; g_device_calls++; }
    void freed(void*) override { g_frees++; g_device_calls++; }
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
// m records whose every double is `value` (the stub kernel does no arithmetic with them)
std::vector<double> table(uint32_t m, double value) { return std::vector<double>(size_t(m) * RPT_TEMPORAL_MOTION_DOUBLES, value); }
}  // namespace

namespace rptg {
hipError_t launch_temporal_accumulate(const TemporalArgs& a, hipStream_t st) {
    const size_t n = size_t(a.width) * a.height;
    volatile double sink = sum(a.rgb, 3 * n) + sum(a.depth, 3 * n) + sum(a.hist_in, n * kTemporalRecDoubles);
    if (a.var) sink = sink + sum(a.var, n);
    if (a.normal) sink = sink + sum(a.normal, 3 * n);
    (void)sink;
    const double total = a.motion ? sum(a.motion, size_t(a.n_motion) * kTemporalMotionDoubles) : 0.0;
    g_seen.push_back({a, st, a.motion ? a.motion[0] : 0.0, total, g_waits});
    for (size_t i = 0; i < 3 * n; i++) a.out_rgb[i] = a.rgb[i] + 1.0;
    for (size_t i = 0; i < n; i++) {
        if (a.out_var) a.out_var[i] = 2.0;
        if (a.out_len) a.out_len[i] = 3.0;
    }
    for (size_t i = 0; i < n * kTemporalRecDoubles; i++) a.hist_out[i] = 4.0;
    return hipSuccess;
}
hipError_t launch_temporal_motion_upload(void* d_table, const double* records, size_t bytes, hipStream_t st) {
    g_device_calls++;
    g_uploads.push_back({d_table, records, bytes, st, g_waits});
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
    const rpt_temporal_params prm{16, RPT_TEMPORAL_MATCH_ID, 0.1, 0.5};
    rpt_camera cams[3] = {{{0, 0, 10}, {0, 0, -1}, {0, 1, 0}, 0.5, 0, 0}, {{1, 0, 10}, {0, 0, -1}, {0, 1, 0}, 0.5, 0, 0}, {{2, 0, 10}, {0, 0, -1}, {0, 1, 0}, 0.6, 0, 0}};
    std::vector<double> rgb(3 * n, 1.0), var(n, 0.1), normal(3 * n, 0.0), depth(3 * n, 1.0), out(3 * n), out_var(n), out_len(n);
    rpt_temporal* t = rpt_temporal_create(0, w, h);
    auto call = [&](int cam, hipStream_t st) {
        return rpt_temporal_accumulate_device(t, &prm, &cams[cam], rgb.data(), var.data(), normal.data(), depth.data(), out.data(), out_var.data(),
                                              out_len.data(), st);
    };

    // ---- refusals, all before any device call
    {
        const int before = g_device_calls;
        std::vector<double> bad = table(2, 1.0);
        bool ok = rpt_temporal_set_motion(t, nullptr, 2) == RPT_ERR_INVALID && rpt_temporal_set_motion_device(t, nullptr, 2) == RPT_ERR_INVALID;
        for (double v : {double(NAN), double(INFINITY), -double(INFINITY)})
            for (int at : {0, 20, 24, 44}) {
                bad = table(2, 1.0);
                bad[at] = v;
                ok = ok && rpt_temporal_set_motion(t, bad.data(), 2) == RPT_ERR_INVALID && std::string(rpt_last_error()).find("finite") != std::string::npos;
            }
        bad = table(2, 1.0);
        ok = ok && rpt_temporal_set_motion(nullptr, bad.data(), 2) == RPT_ERR_INVALID && rpt_temporal_set_motion_device(nullptr, bad.data(), 2) == RPT_ERR_INVALID;
        expect(ok && g_device_calls == before, "NULL records with a count, a value that is not finite and a null handle are refused before any device call");
        bad[21] = bad[22] = bad[23] = NAN;
        bad[45] = INFINITY;
        expect(rpt_temporal_set_motion(t, bad.data(), 2) == RPT_OK && rpt_temporal_set_motion(t, nullptr, 0) == RPT_OK && g_device_calls == before,
               "the three padding doubles are never read; setting and clearing touch no device");
    }

    // ---- a table reaches the next launch and no later one; the first frame consumes its table too
    {
        std::vector<double> tb = table(3, 2.0);
        bool ok = rpt_temporal_set_motion(t, tb.data(), 3) == RPT_OK;
        std::fill(tb.begin(), tb.end(), -9.0);                               // the caller's array is free as soon as the call returns
        tb.clear();
        tb.shrink_to_fit();
        ok = ok && call(0, s1) == RPT_OK && call(1, s2) == RPT_OK;
        expect(ok && g_seen.size() == 2 && g_seen[0].a.have_history == 0 && g_seen[0].a.motion && g_seen[0].a.n_motion == 3 && g_seen[0].first == 2.0 &&
                       g_seen[0].total == 2.0 * 72 && g_seen[1].a.motion == nullptr && g_seen[1].a.n_motion == 0 && g_uploads.size() == 1,
               "a table set before the first frame is consumed by it, copied at set time, and not seen by the next call");
        expect(g_uploads.size() == 1 && g_uploads[0].st == s1 && g_uploads[0].bytes == 3 * 192 && g_uploads[0].dst == g_seen[0].a.motion,
               "the upload goes to the consuming call's stream and is what the kernel reads");
    }

    // ---- ordering: the upload of a later call is enqueued behind the wait for its predecessor's event
    {
        const std::vector<double> tb = table(3, 5.0);
        const int waits = g_waits;
        const bool ok = rpt_temporal_set_motion(t, tb.data(), 3) == RPT_OK && g_waits == waits && g_uploads.size() == 1 && call(2, s1) == RPT_OK;
        expect(ok && g_uploads.size() == 2 && g_uploads[1].waits_before == waits + 1 && g_seen.back().waits_before == waits + 1 && g_uploads[1].st == s1 &&
                       g_seen.back().first == 5.0,
               "set_motion itself reaches no device; the upload follows the wait for the predecessor's event on the call's stream");
        expect(g_uploads[1].src != tb.data() && g_uploads[1].src != g_uploads[0].src,
               "the upload reads the accumulator's own copy, and never the copy an earlier upload read");
    }

    // ---- a refused call leaves the table, a second set replaces the first
    {
        const std::vector<double> a = table(2, 6.0), b = table(4, 7.0);
        const size_t launches = g_seen.size();
        bool ok = rpt_temporal_set_motion(t, a.data(), 2) == RPT_OK;
        rpt_temporal_params bad = prm;
        bad.max_history = 0;
        ok = ok && rpt_temporal_accumulate_device(t, &bad, &cams[0], rgb.data(), nullptr, normal.data(), depth.data(), out.data(), nullptr, nullptr, s1) == RPT_ERR_INVALID;
        ok = ok && rpt_temporal_accumulate_device(t, &prm, &cams[0], rgb.data(), nullptr, nullptr, depth.data(), out.data(), nullptr, nullptr, s1) == RPT_ERR_INVALID;
        ok = ok && g_seen.size() == launches && call(0, s2) == RPT_OK;
        expect(ok && g_seen.back().first == 6.0 && g_seen.back().a.n_motion == 2 && g_seen.back().total == 6.0 * 48, "a refused call leaves the table for the next one");
        ok = rpt_temporal_set_motion(t, a.data(), 2) == RPT_OK && rpt_temporal_set_motion(t, b.data(), 4) == RPT_OK && call(1, s1) == RPT_OK;
        expect(ok && g_seen.back().first == 7.0 && g_seen.back().a.n_motion == 4 && g_seen.back().total == 7.0 * 96, "a second set replaces the first");
        ok = rpt_temporal_set_motion(t, b.data(), 4) == RPT_OK && rpt_temporal_set_motion(t, nullptr, 0) == RPT_OK && call(2, s1) == RPT_OK;
        expect(ok && g_seen.back().a.motion == nullptr && g_seen.back().a.n_motion == 0, "NULL / 0 clears");
    }

    // ---- reset drops it
    {
        const std::vector<double> a = table(2, 8.0);
        uint32_t frames = 9;
        const bool ok = rpt_temporal_set_motion(t, a.data(), 2) == RPT_OK && rpt_temporal_reset(t) == RPT_OK && call(0, s1) == RPT_OK &&
                        rpt_temporal_frames(t, &frames) == RPT_OK;
        expect(ok && frames == 1 && g_seen.back().a.motion == nullptr && g_seen.back().a.have_history == 0, "a reset drops the table");
    }

    // ---- a growing table reallocates (the old block is freed: LeakSanitizer sees one that is not), a smaller one does not
    {
        const int allocs = g_allocs, frees = g_frees;
        bool ok = true;
        const double* last = nullptr;
        for (uint32_t m : {8u, 70u, 1000u, 5u}) {
            const std::vector<double> tb = table(m, double(m));
            ok = ok && rpt_temporal_set_motion(t, tb.data(), m) == RPT_OK && call(1, s1) == RPT_OK && g_seen.back().a.n_motion == m &&
                 g_seen.back().first == double(m) && g_seen.back().total == double(m) * m * 24;
            if (m == 5) ok = ok && g_seen.back().a.motion == last;
            last = g_seen.back().a.motion;
        }
        expect(ok && g_allocs == allocs + 3 && g_frees == frees + 3, "a growing table reallocates, freeing the old block; a smaller one reuses it");
    }

    // ---- the device variant passes the caller's pointer through, uploads nothing, and is one-shot too
    {
        const std::vector<double> dev = table(6, 3.0);
        const size_t uploads = g_uploads.size();
        bool ok = rpt_temporal_set_motion_device(t, dev.data(), 6) == RPT_OK && call(0, s2) == RPT_OK;
        ok = ok && g_seen.back().a.motion == dev.data() && g_seen.back().a.n_motion == 6 && g_seen.back().total == 3.0 * 144 && g_uploads.size() == uploads;
        ok = ok && call(1, s2) == RPT_OK && g_seen.back().a.motion == nullptr;
        expect(ok, "the device variant hands the kernel the caller's table, for one call");
        const std::vector<double> host = table(2, 1.5);
        ok = rpt_temporal_set_motion_device(t, dev.data(), 6) == RPT_OK && rpt_temporal_set_motion(t, host.data(), 2) == RPT_OK && call(2, s1) == RPT_OK;
        ok = ok && g_seen.back().a.motion != dev.data() && g_seen.back().first == 1.5 && g_seen.back().a.n_motion == 2;
        ok = ok && rpt_temporal_set_motion(t, host.data(), 2) == RPT_OK && rpt_temporal_set_motion_device(t, dev.data(), 6) == RPT_OK && call(0, s1) == RPT_OK;
        expect(ok && g_seen.back().a.motion == dev.data() && g_seen.back().a.n_motion == 6, "host and device sets replace each other");
        expect(rpt_temporal_set_motion_device(t, nullptr, 0) == RPT_OK && call(1, s1) == RPT_OK && g_seen.back().a.motion == nullptr, "NULL / 0 clears the device variant");
    }

    // ---- the host entry point and the frame image consume the table as well; a refused frame image leaves it
    {
        const std::vector<double> a = table(2, 4.5);
        bool ok = rpt_temporal_set_motion(t, a.data(), 2) == RPT_OK &&
                  rpt_temporal_accumulate(t, &prm, &cams[1], rgb.data(), var.data(), normal.data(), depth.data(), out.data(), out_var.data(), out_len.data()) == RPT_OK;
        expect(ok && g_seen.back().first == 4.5 && g_seen.back().a.rgb != rgb.data() && g_uploads.back().st == nullptr, "the host entry point consumes the table");
        rpt_buffer* b = rpt_buffer_create(0, w, h, 0);
        std::vector<uint8_t> img(3 * n, 0);
        const size_t launches = g_seen.size();
        ok = rpt_temporal_set_motion(t, a.data(), 2) == RPT_OK &&
             rpt_temporal_frame_image(t, &prm, &cams[0], b, nullptr, nullptr, nullptr, normal.data(), depth.data(), img.data()) == RPT_ERR_STATE &&
             g_seen.size() == launches;
        rpt_buffer_add_samples(b, rgb.data());
        rpt_buffer_add_samples(b, rgb.data());
        ok = ok && rpt_temporal_frame_image(t, &prm, &cams[0], b, nullptr, nullptr, nullptr, normal.data(), depth.data(), img.data()) == RPT_OK;
        expect(ok && g_seen.size() == launches + 1 && g_seen.back().first == 4.5 && g_seen.back().a.n_motion == 2 && img[0] == 125,
               "a refused frame image leaves the table, the next one consumes it");
        ok = rpt_temporal_frame_image(t, &prm, &cams[0], b, nullptr, nullptr, nullptr, normal.data(), depth.data(), img.data()) == RPT_OK;
        expect(ok && g_seen.back().a.motion == nullptr, "and the frame image after that sees none");
        rpt_buffer_destroy(b);
    }

    // ---- record swap and event waits, as temporal_harness.cpp observes them: every call but the first waits once, records once
    {
        bool swap = true;
        for (size_t k = 1; k < g_seen.size(); k++)
            swap = swap && g_seen[k].a.hist_in == g_seen[k - 1].a.hist_out && g_seen[k].a.hist_out == g_seen[k - 1].a.hist_in && g_seen[k].a.hist_in != g_seen[k].a.hist_out;
        expect(swap, "the two record arrays swap per call, with a table or without");
        expect(g_records == int(g_seen.size()) && g_waits == int(g_seen.size()) - 1, "every call but the first waits for its predecessor's event and records its own");
    }

    // a table that is set and never consumed goes with the accumulator
    const std::vector<double> last = table(9, 1.0);
    expect(rpt_temporal_set_motion(t, last.data(), 9) == RPT_OK, "a table may be left unconsumed");
    rpt_temporal_destroy(t);
    g_stub_observer = nullptr;
    std::printf("launches=%zu uploads=%zu waits=%d records=%d failures=%d\n", g_seen.size(), g_uploads.size(), g_waits, g_records, g_failures);
    return g_failures ? 1 : 0;
}

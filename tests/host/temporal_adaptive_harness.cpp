// Test infrastructure for tests/test_host_temporal_adaptive.py: the host half of rpt_temporal_preview_device,
// rpt_temporal_tile_errors_device and rpt_render_adaptive_temporal in the real rpt_capi.cpp over malloc-backed HIP stubs (hip_stubs.h;
// flatten_harness.cpp's launcher stubs are reused), run as a program of its own under AddressSanitizer + UBSan and plain.  Every kernel
// launcher of the loop is a stub that writes one line to a log; the selection stub plays a script of shrinking lists.  main() checks
// the order of the three entry points' refusals (all before any device call), that a preview consumes neither the motion table nor the
// frame count and does not swap the records, that a host table is uploaded once however many calls read it, the loop's call sequence
// round by round, and the life of the active list.  Prints one line per check; exit code 1 on a failure.
#define main flatten_harness_main
#include "flatten_harness.cpp"
#undef main

#include <cmath>
#include <string>
#include <vector>

namespace {
std::vector<std::string> g_log;
std::vector<std::vector<uint32_t>> g_script;           // the lists the selection stub returns, round by round (then: nothing)
size_t g_round = 0;
rptg::TemporalArgs g_last{};
int g_failures = 0, g_device_calls = 0, g_uploads = 0, g_waits = 0, g_records = 0;
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
void expect(bool ok, const char* what) {
    std::printf("%s: %s\n", what, ok ? "ok" : "FAILED");
    if (!ok) g_failures++;
}
bool said(const char* word) { return std::string(rpt_last_error()).find(word) != std::string::npos; }
std::string list_text(const uint32_t* tiles, uint32_t n) {
    if (!tiles) return "all";
    std::string s = "[";
    for (uint32_t i = 0; i < n; i++) s += (i ? " " : "") + std::to_string(tiles[i]);   // (reads every entry: ASan sees a short list)
    return s + "]";
}
}  // namespace

namespace rptg {
hipError_t launch_temporal_accumulate(const TemporalArgs& a, hipStream_t) {
    g_device_calls++;
    g_last = a;
    g_log.push_back("accumulate motion=" + std::to_string(a.n_motion) + " history=" + std::to_string(a.have_history));
    const size_t n = size_t(a.width) * a.height;
    for (size_t i = 0; i < 3 * n; i++) a.out_rgb[i] = a.rgb[i];
    for (size_t i = 0; i < n * kTemporalRecDoubles; i++) a.hist_out[i] = 4.0;
    return hipSuccess;
}
hipError_t launch_temporal_preview(const TemporalArgs& a, const uint32_t* tiles, uint32_t n_tiles, hipStream_t) {
    g_device_calls++;
    g_last = a;
    g_log.push_back("preview " + list_text(tiles, n_tiles) + " motion=" + std::to_string(a.n_motion) + " history=" + std::to_string(a.have_history));
    const size_t n = size_t(a.width) * a.height;
    volatile double sink = a.rgb[3 * n - 1] + a.depth[3 * n - 1] + a.hist_in[n * kTemporalRecDoubles - 1] + (a.var ? a.var[n - 1] : 0.0) +
                           (a.motion ? a.motion[size_t(a.n_motion) * kTemporalMotionDoubles - 1] : 0.0);
    (void)sink;
    a.out_rgb[3 * n - 1] = 1.0;
    if (a.out_var) a.out_var[n - 1] = 1.0;
    return hipSuccess;
}
hipError_t launch_temporal_motion_upload(void* d_table, const double* records, size_t bytes, hipStream_t) {
    g_device_calls++;
    g_uploads++;
    std::memcpy(d_table, records, bytes);
    return hipSuccess;
}
hipError_t launch_buffer_mean(uint32_t n_pixels, uint32_t n_batches, const double*, const double*, double* rgb, double* var, hipStream_t) {
    g_log.push_back("mean batches=" + std::to_string(n_batches));
    rgb[3 * size_t(n_pixels) - 1] = 0.25;
    if (var) var[n_pixels - 1] = 0.5;
    return hipSuccess;
}
hipError_t launch_buffer_mean_tiles(const TileBufferView& b, const double*, const double*, double* rgb, double* var, hipStream_t) {
    g_log.push_back("mean tiles batches=" + std::to_string(b.n_batches));
    rgb[3 * size_t(b.width) * b.height - 1] = 0.25;
    if (var) var[size_t(b.width) * b.height - 1] = 0.5;
    return hipSuccess;
}
hipError_t launch_color_bytes(uint64_t n_values, const double*, uint8_t* out, hipStream_t) {
    out[n_values - 1] = 1;
    return hipSuccess;
}
hipError_t launch_plane_tile_errors(uint32_t width, uint32_t height, double, const double* rgb, const double* var, const uint32_t* tiles, uint32_t n_tiles,
                                    double* err, hipStream_t) {
    g_device_calls++;
    g_log.push_back("errors " + list_text(tiles, n_tiles));
    volatile double sink = rgb[3 * size_t(width) * height - 1] + var[size_t(width) * height - 1];
    (void)sink;
    err[((width + 31) / 32) * ((height + 31) / 32) - 1] = 1.0;
    return hipSuccess;
}
hipError_t launch_tile_select_list(const TileBufferView& b, double, uint32_t, const double* err, const uint32_t* in, uint32_t n_in, uint32_t* out,
                                   uint32_t* n_out, hipStream_t) {
    g_device_calls++;
    g_log.push_back("select " + list_text(in, n_in) + (in && in == out ? " in place" : ""));
    volatile double sink = err[b.tiles_x * b.tiles_y - 1];
    (void)sink;
    const std::vector<uint32_t> next = g_round < g_script.size() ? g_script[g_round] : std::vector<uint32_t>();
    g_round++;
    for (size_t i = 0; i < next.size(); i++) out[i] = next[i];
    *n_out = uint32_t(next.size());
    return hipSuccess;
}
hipError_t launch_buffer_add_tiles(const TileBufferView&, const double*, double*, double*, uint32_t* extra, const uint32_t* tiles, uint32_t n_tiles,
                                   hipStream_t) {
    g_log.push_back("add " + list_text(tiles, n_tiles));
    for (uint32_t i = 0; i < n_tiles; i++) extra[tiles[i]] += 1;
    return hipSuccess;
}
}  // namespace rptg

int main() {
    Watch watch;
    g_stub_observer = &watch;
    const uint32_t w = 70, h = 40;                                              // 3 x 2 tiles
    const size_t n = size_t(w) * h;
    hipStream_t const s1 = reinterpret_cast<hipStream_t>(uintptr_t(0x100));
    const rpt_temporal_params tp{16, RPT_TEMPORAL_MATCH_ID, 0.1, 0.5};
    rpt_camera cam{{0, 0, 10}, {0, 0, -1}, {0, 1, 0}, 0.5, 0, 0};
    std::vector<double> rgb(3 * n, 1.0), var(n, 0.1), normal(3 * n, 0.0), depth(3 * n, 1.0), out(3 * n), out_var(n), out_len(n), err(6);
    std::vector<uint32_t> ids = {4, 1, 9};
    rpt_temporal* t = rpt_temporal_create(0, w, h);
    auto preview = [&](rpt_temporal* acc, const void* tiles, uint32_t n_tiles) {
        return rpt_temporal_preview_device(acc, &tp, &cam, rgb.data(), var.data(), normal.data(), depth.data(), tiles, n_tiles, out.data(), out_var.data(),
                                           out_len.data(), s1);
    };
    auto accumulate = [&]() {
        return rpt_temporal_accumulate_device(t, &tp, &cam, rgb.data(), var.data(), normal.data(), depth.data(), out.data(), out_var.data(), out_len.data(), s1);
    };

    // ---- the preview's refusals: the accumulation's, then the list, then the handle, then the list's length; no device call
    {
        const int before = g_device_calls;
        rpt_temporal_params bad = tp;
        bad.max_history = 0;
        bool ok = rpt_temporal_preview_device(t, &bad, &cam, nullptr, nullptr, nullptr, nullptr, nullptr, 3, nullptr, nullptr, nullptr, s1) == RPT_ERR_INVALID &&
                  said("max_history");
        ok = ok && rpt_temporal_preview_device(t, &tp, &cam, rgb.data(), var.data(), normal.data(), depth.data(), nullptr, 3, out.data(), out.data(), nullptr, s1) ==
                       RPT_ERR_INVALID && said("outputs must differ");
        ok = ok && preview(nullptr, nullptr, 3) == RPT_ERR_INVALID && said("null tile list");
        ok = ok && preview(nullptr, ids.data(), 3) == RPT_ERR_INVALID && said("null accumulator");
        ok = ok && preview(t, nullptr, 3) == RPT_ERR_INVALID && said("null tile list");
        std::vector<uint32_t> many(7, 0);
        ok = ok && preview(t, many.data(), 7) == RPT_ERR_INVALID && said("more tiles");
        expect(ok && g_device_calls == before && g_log.empty(), "preview: parameters, planes, a null list, the handle, the list's length, in this order, before any device call");
    }
    // ---- the tile errors' refusals
    {
        const int before = g_device_calls;
        bool ok = rpt_temporal_tile_errors_device(nullptr, nullptr, nullptr, 0.0, nullptr, 3, nullptr, s1) == RPT_ERR_INVALID && said("floor");
        ok = ok && rpt_temporal_tile_errors_device(t, rgb.data(), var.data(), INFINITY, ids.data(), 3, err.data(), s1) == RPT_ERR_INVALID && said("floor");
        ok = ok && rpt_temporal_tile_errors_device(nullptr, rgb.data(), var.data(), 0.1, nullptr, 3, err.data(), s1) == RPT_ERR_INVALID && said("null argument");
        ok = ok && rpt_temporal_tile_errors_device(t, rgb.data(), nullptr, 0.1, nullptr, 3, err.data(), s1) == RPT_ERR_INVALID && said("null argument");
        ok = ok && rpt_temporal_tile_errors_device(t, rgb.data(), var.data(), 0.1, nullptr, 3, err.data(), s1) == RPT_ERR_INVALID && said("null tile list");
        std::vector<uint32_t> many(7, 0);
        ok = ok && rpt_temporal_tile_errors_device(t, rgb.data(), var.data(), 0.1, many.data(), 7, err.data(), s1) == RPT_ERR_INVALID && said("more tiles");
        expect(ok && g_device_calls == before && g_log.empty(), "tile errors: floor, pointers, a null list, the list's length, in this order, before any device call");
        ok = rpt_temporal_tile_errors_device(t, rgb.data(), var.data(), 0.1, ids.data(), 3, err.data(), s1) == RPT_OK && g_log.back() == "errors [4 1 9]";
        ok = ok && rpt_temporal_tile_errors_device(t, rgb.data(), var.data(), 0.1, nullptr, 0, err.data(), s1) == RPT_OK && g_log.back() == "errors all";
        expect(ok && g_waits == 0 && g_records == 0, "tile errors: the list arrives; the accumulator's event is neither waited for nor recorded");
        g_log.clear();
    }
    // ---- a preview consumes nothing
    {
        uint32_t frames = 9;
        const std::vector<double> table(2 * RPT_TEMPORAL_MOTION_DOUBLES, 1.0);
        bool ok = accumulate() == RPT_OK && rpt_temporal_frames(t, &frames) == RPT_OK && frames == 1;
        const double* const hist_in_next = g_last.hist_out;
        ok = ok && rpt_temporal_set_motion(t, table.data(), 2) == RPT_OK;
        const int waits = g_waits, records = g_records;
        ok = ok && preview(t, nullptr, 0) == RPT_OK && g_log.back() == "preview all motion=2 history=1" && g_last.hist_in == hist_in_next;
        ok = ok && preview(t, ids.data(), 3) == RPT_OK && g_log.back() == "preview [4 1 9] motion=2 history=1" && g_last.hist_in == hist_in_next;
        ok = ok && preview(t, ids.data(), 0) == RPT_OK && g_log.back() == "preview [] motion=2 history=1";
        ok = ok && rpt_temporal_frames(t, &frames) == RPT_OK && frames == 1;
        expect(ok && g_waits == waits + 3 && g_records == records + 3, "previews read the table and the history, keep the frame count, and are ordered through the event");
        ok = accumulate() == RPT_OK && g_log.back() == "accumulate motion=2 history=1" && g_last.hist_in == hist_in_next && g_uploads == 1;
        expect(ok, "the accumulation behind them reads the same records and the same table, which was uploaded once");
        ok = preview(t, nullptr, 0) == RPT_OK && g_log.back() == "preview all motion=0 history=1" && accumulate() == RPT_OK &&
             g_log.back() == "accumulate motion=0 history=1" && rpt_temporal_frames(t, &frames) == RPT_OK && frames == 3;
        expect(ok, "the table was consumed exactly once");
        ok = rpt_temporal_set_motion(t, table.data(), 2) == RPT_OK && preview(t, nullptr, 0) == RPT_OK && rpt_temporal_set_motion(t, table.data(), 1) == RPT_OK &&
             preview(t, nullptr, 0) == RPT_OK && g_log.back() == "preview all motion=1 history=1" && g_uploads == 3;
        ok = ok && rpt_temporal_reset(t) == RPT_OK && preview(t, nullptr, 0) == RPT_OK && g_log.back() == "preview all motion=0 history=0";
        expect(ok, "a second set replaces a table a preview has uploaded; a reset drops it");
        g_log.clear();
    }
    // ---- the loop
    {
        rpt_scene* s = rpt_scene_create();
        add(s, rpt::sphere());
        rpt_scene_commit(s, 0);
        rpt_render_params prm{};
        prm.width = w; prm.height = h; prm.max_bounces = 2; prm.shard_count = 1;
        const rpt_adaptive_params ap{2, 2, 6, 0, 0.1, 0.05};
        rpt_buffer* b = rpt_buffer_create(0, w, h, 0);
        uint64_t stats[4] = {9, 9, 9, 9};
        const std::vector<double> table(3 * RPT_TEMPORAL_MOTION_DOUBLES, 1.0);
        auto loop = [&](rpt_buffer* buf, rpt_temporal* acc, const rpt_adaptive_params& a, uint32_t offset, const void* nrm, const void* dpt) {
            return rpt_render_adaptive_temporal(s, &cam, &prm, &a, 1, offset, buf, acc, &tp, nrm, dpt, stats);
        };
        // refusals, in order, before any device call
        rpt_buffer* other = rpt_buffer_create(0, w, h + 1, 0);
        rpt_temporal* small = rpt_temporal_create(0, w, h + 1);
        const int before = g_device_calls;
        rpt_adaptive_params bad = ap;
        bad.min_batches = 1;
        bool ok = loop(nullptr, nullptr, bad, 0xFFFFFFFFu, nullptr, nullptr) == RPT_ERR_INVALID && said("min_batches");
        ok = ok && loop(nullptr, nullptr, ap, 0xFFFFFFFFu - 11, nullptr, nullptr) == RPT_ERR_INVALID && said("sample_offset");
        ok = ok && loop(nullptr, nullptr, ap, 0, nullptr, nullptr) == RPT_ERR_INVALID && said("null buffer");
        ok = ok && loop(other, nullptr, ap, 0, nullptr, nullptr) == RPT_ERR_INVALID && said("dimension");
        ok = ok && loop(b, nullptr, ap, 0, normal.data(), nullptr) == RPT_ERR_INVALID && said("depth plane");
        ok = ok && loop(b, nullptr, ap, 0, nullptr, depth.data()) == RPT_ERR_INVALID && said("needs the normal");
        ok = ok && loop(b, nullptr, ap, 0, normal.data(), depth.data()) == RPT_ERR_INVALID && said("null accumulator");
        ok = ok && loop(b, small, ap, 0, normal.data(), depth.data()) == RPT_ERR_INVALID && said("different sizes");
        expect(ok && g_device_calls == before && g_log.empty() && stats[0] == 9,
               "loop: adaptive parameters, the offset, the buffer, the temporal planes, the handle, the sizes, in this order, before any device call");
        rpt_buffer_destroy(other);
        rpt_temporal_destroy(small);

        // the call sequence: all -> [1 3 4] -> [3 4] -> [4] -> max_batches ends the loop
        ok = accumulate() == RPT_OK && rpt_temporal_set_motion(t, table.data(), 3) == RPT_OK;
        g_log.clear();
        g_script = {{1, 3, 4}, {3, 4}, {4}, {4}};
        g_round = 0;
        const int uploads = g_uploads;
        ok = ok && loop(b, t, ap, 100, normal.data(), depth.data()) == RPT_OK;
        const std::vector<std::string> want = {
            "mean batches=2", "preview all motion=3 history=1", "errors all", "select all", "add [1 3 4]",
            "mean tiles batches=2", "preview [1 3 4] motion=3 history=1", "errors [1 3 4]", "select [1 3 4] in place", "add [3 4]",
            "mean tiles batches=2", "preview [3 4] motion=3 history=1", "errors [3 4]", "select [3 4] in place", "add [4]",
            "mean tiles batches=2", "preview [4] motion=3 history=1", "errors [4]", "select [4] in place", "add [4]"};
        for (size_t i = 0; i < g_log.size(); i++) std::printf("  %s\n", g_log[i].c_str());
        expect(ok && g_log == want, "loop: mean, preview, errors, selection and tile batch, round by round; the active list only shrinks; max_batches ends it");
        expect(stats[0] == 4 && stats[1] == 2 * 6 + 3 + 2 + 1 + 1 && stats[2] == 1 && stats[3] == 6 && g_uploads == uploads + 1,
               "loop: the stats; the table was uploaded once for all rounds");
        uint32_t frames = 0;
        std::vector<uint32_t> counts(6);
        ok = rpt_temporal_frames(t, &frames) == RPT_OK && frames == 1 && rpt_buffer_tile_batches(b, counts.data(), 6) == RPT_OK &&
             counts == std::vector<uint32_t>({2, 3, 2, 4, 6, 2});
        ok = ok && accumulate() == RPT_OK && g_log.back() == "accumulate motion=3 history=1" && g_uploads == uploads + 1;
        expect(ok, "loop: the frame count and the table are as before; the accumulation that follows consumes the table");
        ok = loop(b, t, ap, 0, normal.data(), depth.data()) == RPT_ERR_STATE && said("empty buffer");
        expect(ok, "loop: a used buffer is refused");

        // nothing selected in the first round: no tile batch at all
        rpt_buffer* fresh = rpt_buffer_create(0, w, h, 0);
        g_log.clear();
        g_script.clear();
        g_round = 0;
        ok = loop(fresh, t, ap, 0, normal.data(), depth.data()) == RPT_OK && stats[0] == 0 && stats[1] == 12 && stats[2] == 0;
        expect(ok && g_log == std::vector<std::string>({"mean batches=2", "preview all motion=0 history=1", "errors all", "select all"}),
               "loop: a round that selects nothing ends it");
        rpt_buffer_destroy(fresh);
        rpt_buffer_destroy(b);
        rpt_scene_destroy(s);
    }
    rpt_temporal_destroy(t);
    g_stub_observer = nullptr;
    std::printf("failures=%d\n", g_failures);
    return g_failures ? 1 : 0;
}

// Test infrastructure for tests/test_upsample_host.py: the host half of rpt_upsample*, rpt_image_bytes_device and
// rpt_buffer_upsampled_image in the real rpt_capi.cpp over malloc-backed HIP stubs (hip_stubs.h; flatten_harness.cpp's launcher stubs
// are reused), run as a program of its own under AddressSanitizer + UBSan and plain.  The stub of the upsampling kernel reads and
// writes every byte the kernel would (every plane it is handed, both outputs), so an array that is too small or freed is a sanitizer
// report; it records its arguments, and main() checks every refusal in the order include/rpt_hip.h states, that a refused call
// reaches no launch, the host entry point's copies and the pipeline of rpt_buffer_upsampled_image.  Prints one line per check; exit
// code 1 on a failure.
#define main flatten_harness_main
#include "flatten_harness.cpp"
#undef main

#include <string>
#include <vector>

namespace {
std::vector<rptg::UpsampleArgs> g_seen;
std::vector<hipStream_t> g_streams;
int g_failures = 0, g_denoise_passes = 0, g_bytes = 0;
double sum(const double* p, size_t n) {
    double s = 0;
    for (size_t i = 0; i < n; i++) s += p[i];
    return s;
}
void expect(bool ok, const char* what) {
    std::printf("%s: %s\n", what, ok ? "ok" : "FAILED");
    if (!ok) g_failures++;
}
bool refused(int rc, const char* text) { return rc == RPT_ERR_INVALID && std::string(rpt_last_error()).find(text) != std::string::npos; }
}  // namespace

namespace rptg {
// Touches what upsample_kernel touches; out = the footprint pixel's colour + 1, the variance plane 2.
hipError_t launch_upsample(const UpsampleArgs& a, hipStream_t st) {
    g_seen.push_back(a);
    g_streams.push_back(st);
    const size_t n = size_t(a.width) * a.height, N = n * a.scale * a.scale;
    volatile double sink = sum(a.lo_rgb, 3 * n);
    if (a.lo_var) sink = sink + sum(a.lo_var, n);
    for (const double* p : {a.lo_albedo, a.lo_normal, a.lo_depth})
        if (p) sink = sink + sum(p, 3 * n);
    for (const double* p : {a.hi_albedo, a.hi_normal, a.hi_depth})
        if (p) sink = sink + sum(p, 3 * N);
    (void)sink;
    const size_t W = size_t(a.width) * a.scale;
    for (size_t p = 0; p < N; p++) {
        const size_t q = (p / W / a.scale) * a.width + (p % W) / a.scale;
        for (int k = 0; k < 3; k++) a.out_rgb[3 * p + k] = a.lo_rgb[3 * q + k] + 1.0;
        if (a.out_var) a.out_var[p] = 2.0;
    }
    return hipSuccess;
}
hipError_t launch_buffer_mean(uint32_t n_pixels, uint32_t, const double*, const double*, double* rgb, double* var, hipStream_t) {
    for (size_t i = 0; i < 3 * size_t(n_pixels); i++) rgb[i] = 0.25;
    if (var)
        for (size_t i = 0; i < n_pixels; i++) var[i] = 0.5;
    return hipSuccess;
}
hipError_t launch_color_bytes(uint64_t n_values, const double* rgb, uint8_t* out, hipStream_t) {
    g_bytes++;
    for (uint64_t i = 0; i < n_values; i++) out[i] = uint8_t(rgb[i] * 100.0);
    return hipSuccess;
}
hipError_t launch_denoise_prepare(const DenoisePrepareArgs& a, hipStream_t) {
    (void)sum(a.rgb, 3 * size_t(a.n_pixels));
    return hipSuccess;
}
// The last pass writes the frame it was given at the start, halved: 0.25 -> 0.125.
hipError_t launch_denoise_pass(const DenoisePassArgs& a, bool, hipStream_t) {
    g_denoise_passes++;
    if (a.out)
        for (size_t i = 0; i < 3 * size_t(a.width) * a.height; i++) a.out[i] = 0.125;
    return hipSuccess;
}
}  // namespace rptg

int main() {
    const uint32_t w = 5, h = 3, s = 2;
    const size_t n = size_t(w) * h, N = n * s * s;
    hipStream_t const s1 = reinterpret_cast<hipStream_t>(uintptr_t(0x100));
    // exact sizes on the heap: a read or a write past a plane is a sanitizer report
    std::vector<double> rgb(3 * n, 1.0), var(n, 0.1), la(3 * n, 0.5), ln(3 * n, 0.0), ld(3 * n, 1.0), ha(3 * N, 0.5), hn(3 * N, 0.0), hd(3 * N, 1.0),
        out(3 * N), out_var(N);
    const rpt_upsample_params all{s, 1, RPT_UPSAMPLE_DEMODULATE | RPT_UPSAMPLE_MATCH_ID, 0, 0.5, 0.3};
    const rpt_upsample_params none{s, 1, 0, 0, 0.0, 0.0};
    auto dev = [&](const rpt_upsample_params* p, uint32_t ww, uint32_t hh, const double* a0, const double* a1, const double* a2, const double* a3,
                   const double* a4, const double* a5, const double* a6, const double* a7, double* o, double* ov) {
        return rpt_upsample_device(p, ww, hh, a0, a1, a2, a3, a4, a5, a6, a7, o, ov, s1);
    };
    auto host = [&](const rpt_upsample_params* p, uint32_t ww, uint32_t hh, const double* a0, const double* a1, const double* a2, const double* a3,
                    const double* a4, const double* a5, const double* a6, const double* a7, double* o, double* ov) {
        return rpt_upsample(0, p, ww, hh, a0, a1, a2, a3, a4, a5, a6, a7, o, ov);
    };

    // ---- every refusal, in the stated order: each call below is wrong in the named way AND in every way that is checked later
    for (int which = 0; which < 2; which++) {
        auto call = [&](const rpt_upsample_params* p, uint32_t ww, uint32_t hh, const double* a0, const double* a1, const double* a2, const double* a3,
                        const double* a4, const double* a5, const double* a6, const double* a7, double* o, double* ov) {
            return which ? host(p, ww, hh, a0, a1, a2, a3, a4, a5, a6, a7, o, ov) : dev(p, ww, hh, a0, a1, a2, a3, a4, a5, a6, a7, o, ov);
        };
        rpt_upsample_params p = all;
        bool ok = refused(call(nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "parameters");
        p.scale = 5; p.radius = 0; p.flags = 4; p.sigma_normal = -1.0;
        ok = ok && refused(call(&p, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "scale");
        p.scale = 1;
        ok = ok && refused(call(&p, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "scale");
        p.scale = 4;
        ok = ok && refused(call(&p, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "radius");
        p.radius = 3;
        ok = ok && refused(call(&p, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "radius");
        p.radius = 2;
        ok = ok && refused(call(&p, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "flag");
        p.flags = 3;
        ok = ok && refused(call(&p, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "sigma");
        p.sigma_normal = 0.5; p.sigma_depth = std::nan("");
        ok = ok && refused(call(&p, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "sigma");
        p.sigma_depth = INFINITY;
        ok = ok && refused(call(&p, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "sigma");
        p.sigma_depth = 0.3;
        ok = ok && refused(call(&p, 0, h, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "empty");
        ok = ok && refused(call(&p, w, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "empty");
        ok = ok && refused(call(&p, 1u << 30, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "too large");
        ok = ok && refused(call(&p, 1, 1u << 30, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "too large");
        ok = ok && refused(call(&p, 1u << 14, 1u << 13, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "too large");
        expect(ok, which ? "host entry: parameters and sizes, in order" : "device entry: parameters and sizes, in order");
        p = all;
        ok = refused(call(&p, w, h, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "null frame");
        ok = ok && refused(call(&p, w, h, rgb.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "null frame");
        ok = ok && refused(call(&p, w, h, rgb.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, out.data(), nullptr),
                           "sigma_normal > 0 needs the low");
        ok = ok && refused(call(&p, w, h, rgb.data(), nullptr, nullptr, ln.data(), nullptr, nullptr, nullptr, nullptr, out.data(), nullptr),
                           "sigma_normal > 0 needs the full");
        ok = ok && refused(call(&p, w, h, rgb.data(), nullptr, nullptr, ln.data(), nullptr, nullptr, hn.data(), nullptr, out.data(), nullptr),
                           "sigma_depth > 0 needs the low");
        ok = ok && refused(call(&p, w, h, rgb.data(), nullptr, nullptr, ln.data(), ld.data(), nullptr, hn.data(), nullptr, out.data(), nullptr),
                           "sigma_depth > 0 needs the full");
        ok = ok && refused(call(&p, w, h, rgb.data(), nullptr, nullptr, ln.data(), ld.data(), nullptr, hn.data(), hd.data(), out.data(), nullptr),
                           "DEMODULATE needs the low");
        ok = ok && refused(call(&p, w, h, rgb.data(), nullptr, la.data(), ln.data(), ld.data(), nullptr, hn.data(), hd.data(), out.data(), nullptr),
                           "DEMODULATE needs the full");
        p.sigma_depth = 0.0;
        ok = ok && refused(call(&p, w, h, rgb.data(), nullptr, la.data(), ln.data(), nullptr, ha.data(), hn.data(), hd.data(), out.data(), nullptr),
                           "MATCH_ID needs the low");
        ok = ok && refused(call(&p, w, h, rgb.data(), nullptr, la.data(), ln.data(), ld.data(), ha.data(), hn.data(), nullptr, out.data(), nullptr),
                           "MATCH_ID needs the full");
        expect(ok, which ? "host entry: frames and planes, in order" : "device entry: frames and planes, in order");
        p = all;
        const double* ins[8] = {rgb.data(), var.data(), la.data(), ln.data(), ld.data(), ha.data(), hn.data(), hd.data()};
        ok = true;
        for (int k = 0; k < 8; k++) {
            ok = ok && refused(call(&p, w, h, ins[0], ins[1], ins[2], ins[3], ins[4], ins[5], ins[6], ins[7], const_cast<double*>(ins[k]), out_var.data()),
                               "output must not");
            ok = ok && refused(call(&p, w, h, ins[0], ins[1], ins[2], ins[3], ins[4], ins[5], ins[6], ins[7], out.data(), const_cast<double*>(ins[k])),
                               "output must not");
        }
        ok = ok && refused(call(&p, w, h, ins[0], ins[1], ins[2], ins[3], ins[4], ins[5], ins[6], ins[7], out.data(), out.data()), "differ");
        expect(ok, which ? "host entry: an output is no input" : "device entry: an output is no input");
    }
    expect(refused(rpt_upsample(3, &all, w, h, rgb.data(), var.data(), la.data(), ln.data(), ld.data(), ha.data(), hn.data(), hd.data(), out.data(), out_var.data()),
                   "device index") &&
                   refused(rpt_upsample(-1, &none, w, h, rgb.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, out.data(), nullptr), "device index"),
           "host entry: the device index comes last");
    expect(g_seen.empty(), "a refused call reaches no launch");

    // ---- the device entry: the arguments reach the launch; what a term that is off would read is not handed on
    bool ok = dev(&all, w, h, rgb.data(), var.data(), la.data(), ln.data(), ld.data(), ha.data(), hn.data(), hd.data(), out.data(), out_var.data()) == RPT_OK;
    expect(ok && g_seen.size() == 1 && g_streams[0] == s1 && g_seen[0].width == w && g_seen[0].height == h && g_seen[0].scale == s && g_seen[0].radius == 1 &&
                   g_seen[0].flags == 3 && g_seen[0].terms == 3 && g_seen[0].a_n == 1.0 / 0.5 && g_seen[0].a_z == 1.0 / (0.3 * 2.0) &&
                   g_seen[0].lo_rgb == rgb.data() && g_seen[0].lo_var == var.data() && g_seen[0].lo_albedo == la.data() && g_seen[0].lo_normal == ln.data() &&
                   g_seen[0].lo_depth == ld.data() && g_seen[0].hi_albedo == ha.data() && g_seen[0].hi_normal == hn.data() && g_seen[0].hi_depth == hd.data() &&
                   g_seen[0].out_rgb == out.data() && g_seen[0].out_var == out_var.data() && sum(out.data(), 3 * N) == 2.0 * 3 * N &&
                   sum(out_var.data(), N) == 2.0 * N,
           "the launch gets the call's arguments");
    ok = dev(&none, w, h, rgb.data(), nullptr, la.data(), ln.data(), ld.data(), ha.data(), hn.data(), hd.data(), out.data(), nullptr) == RPT_OK;
    expect(ok && g_seen.size() == 2 && g_seen[1].terms == 0 && !g_seen[1].lo_var && !g_seen[1].lo_albedo && !g_seen[1].lo_normal && !g_seen[1].lo_depth &&
                   !g_seen[1].hi_albedo && !g_seen[1].hi_normal && !g_seen[1].hi_depth && !g_seen[1].out_var,
           "with every term and flag off no plane reaches the kernel");
    const rpt_upsample_params id_only{3, 2, RPT_UPSAMPLE_MATCH_ID, 0, 0.0, 0.0};
    {
        std::vector<double> hd3(3 * n * 9, 1.0), out3(3 * n * 9);
        ok = dev(&id_only, w, h, rgb.data(), nullptr, nullptr, nullptr, ld.data(), nullptr, nullptr, hd3.data(), out3.data(), nullptr) == RPT_OK;
        expect(ok && g_seen.back().scale == 3 && g_seen.back().radius == 2 && g_seen.back().lo_depth == ld.data() && g_seen.back().hi_depth == hd3.data() &&
                       !g_seen.back().lo_normal,
               "MATCH_ID alone hands on the depth planes");
    }

    // ---- the host entry point: planes up, outputs down, the optional ones only where given
    std::fill(out.begin(), out.end(), -1.0);
    std::fill(out_var.begin(), out_var.end(), -1.0);
    ok = host(&all, w, h, rgb.data(), var.data(), la.data(), ln.data(), ld.data(), ha.data(), hn.data(), hd.data(), out.data(), out_var.data()) == RPT_OK;
    expect(ok && sum(out.data(), 3 * N) == 2.0 * 3 * N && sum(out_var.data(), N) == 2.0 * N && g_seen.back().lo_rgb != rgb.data() && g_seen.back().lo_var,
           "the host entry point copies the planes up and both outputs down");
    std::fill(out_var.begin(), out_var.end(), -1.0);
    ok = host(&none, w, h, rgb.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, out.data(), nullptr) == RPT_OK;
    expect(ok && sum(out_var.data(), N) == -1.0 * N && !g_seen.back().lo_var && !g_seen.back().out_var, "NULL planes and outputs stay NULL");
    g_stub_malloc_limit = 100;
    expect(host(&none, w, h, rgb.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, out.data(), nullptr) == RPT_ERR_DEVICE,
           "the host entry point survives a failed allocation");
    g_stub_malloc_limit = SIZE_MAX;

    // ---- rpt_image_bytes_device
    std::vector<uint8_t> img(3 * N, 0);
    expect(refused(rpt_image_bytes_device(nullptr, 4, 4, img.data(), nullptr), "null") && refused(rpt_image_bytes_device(out.data(), 4, 4, nullptr, nullptr), "null") &&
                   refused(rpt_image_bytes_device(out.data(), 0, 4, img.data(), nullptr), "size") &&
                   refused(rpt_image_bytes_device(out.data(), 1u << 16, 1u << 15, img.data(), nullptr), "size") && g_bytes == 0,
           "image bytes: refusals before the launch");
    std::fill(out.begin(), out.end(), 0.5);
    expect(rpt_image_bytes_device(out.data(), w * s, h * s, img.data(), s1) == RPT_OK && g_bytes == 1 && img[0] == 50 && img[3 * N - 1] == 50, "image bytes: the plane's bytes come back");

    // ---- rpt_buffer_upsampled_image: a buffer of two batches -> bytes; the checks' order, state, the optional low-resolution filter
    rpt_buffer* b = rpt_buffer_create(0, w, h, 0);
    const size_t before = g_seen.size();
    expect(refused(rpt_buffer_upsampled_image(nullptr, nullptr, nullptr, &all, la.data(), ln.data(), ld.data(), ha.data(), hn.data(), hd.data(), img.data()), "null argument") &&
                   refused(rpt_buffer_upsampled_image(b, nullptr, nullptr, &all, la.data(), ln.data(), ld.data(), ha.data(), hn.data(), hd.data(), nullptr), "null argument") &&
                   refused(rpt_buffer_upsampled_image(b, nullptr, nullptr, nullptr, la.data(), ln.data(), ld.data(), ha.data(), hn.data(), hd.data(), img.data()), "parameters") &&
                   refused(rpt_buffer_upsampled_image(b, nullptr, nullptr, &all, la.data(), ln.data(), ld.data(), ha.data(), nullptr, hd.data(), img.data()),
                           "sigma_normal > 0 needs the full"),
           "upsampled image: the buffer, then the upsampling's checks");
    rpt_denoiser* den = rpt_denoiser_create(0, w, h);
    rpt_denoiser* small = rpt_denoiser_create(0, 3, 3);
    const rpt_denoise_params dprm{2, RPT_DENOISE_MATCH_ID, 4.0, 0.5, 0.0};
    expect(refused(rpt_buffer_upsampled_image(b, den, nullptr, &all, la.data(), ln.data(), ld.data(), ha.data(), hn.data(), hd.data(), img.data()), "null denoise") &&
                   refused(rpt_buffer_upsampled_image(b, small, &dprm, &all, la.data(), ln.data(), ld.data(), ha.data(), hn.data(), hd.data(), img.data()), "sizes"),
           "upsampled image: a denoiser needs its parameters and the buffer's size");
    expect(rpt_buffer_upsampled_image(b, nullptr, nullptr, &all, la.data(), ln.data(), ld.data(), ha.data(), hn.data(), hd.data(), img.data()) == RPT_ERR_STATE &&
                   g_seen.size() == before && g_denoise_passes == 0,
           "fewer than two batches: RPT_ERR_STATE, and nothing is launched");
    rpt_buffer_add_samples(b, rgb.data());
    rpt_buffer_add_samples(b, rgb.data());
    ok = rpt_buffer_upsampled_image(b, nullptr, &dprm, &all, la.data(), ln.data(), ld.data(), ha.data(), hn.data(), hd.data(), img.data()) == RPT_OK;
    expect(ok && g_seen.size() == before + 1 && g_denoise_passes == 0 && img[0] == 125 && img[3 * N - 1] == 125 && g_seen.back().hi_normal == hn.data() &&
                   !g_seen.back().lo_var && !g_seen.back().out_var,
           "upsampled image: mean 0.25 -> upsample (+1) -> bytes; without a denoiser its parameters are ignored");
    ok = rpt_buffer_upsampled_image(b, den, &dprm, &all, la.data(), ln.data(), ld.data(), ha.data(), hn.data(), hd.data(), img.data()) == RPT_OK;
    expect(ok && g_seen.size() == before + 2 && g_denoise_passes == 2 && img[0] == 112 && img[3 * N - 1] == 112,
           "upsampled image: mean -> filter at the low resolution (0.125) -> upsample (+1) -> bytes");
    const rpt_upsample_params four{4, 2, 0, 0, 0.0, 0.0};
    std::vector<uint8_t> img4(3 * n * 16, 0);
    ok = rpt_buffer_upsampled_image(b, nullptr, nullptr, &four, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, img4.data()) == RPT_OK;
    expect(ok && img4[0] == 125 && img4[3 * n * 16 - 1] == 125, "upsampled image: the scratch grows with the scale");

    rpt_denoiser_destroy(small);
    rpt_denoiser_destroy(den);
    rpt_buffer_destroy(b);
    std::printf("launches=%zu denoise_passes=%d byte_launches=%d failures=%d\n", g_seen.size(), g_denoise_passes, g_bytes, g_failures);
    return g_failures ? 1 : 0;
}

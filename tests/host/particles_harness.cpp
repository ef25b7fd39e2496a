// Test infrastructure for tests/test_host_particles.py: the host half of rpt_particles_* in the real rpt_amd/csrc/rpt_particles.cpp over
// malloc-backed HIP stubs (hip_stubs.h), run as a program of its own under AddressSanitizer + UBSan and plain.  The stubs of the two
// launchers read and write every byte the kernels would (both state arrays, the six counters, the display array), so an array that is
// too small or freed is a sanitizer report; they record their arguments, and main() checks the handle's life cycle, the cut of a
// 2,500-step sequence into launches of at most 256 steps with the right last step, the event that orders the calls of one handle,
// the check order, and a set_state issued while an integrate is queued.  Prints one line per check; exit code 1 on a failure.
#include "hip_stubs.h"

#include <cstdio>
#include <string>
#include <vector>

#include "../../rpt_amd/csrc/host_internal.h"
static thread_local std::string g_err;
namespace rpti {
int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
}  // namespace rpti
extern "C" const char* rpt_last_error(void) { return g_err.c_str(); }
#include "../../rpt_amd/csrc/rpt_particles.cpp"

namespace {
struct Seen {
    rptg::ParticlesArgs a;
    uint32_t block, lanes;
    hipStream_t st;
};
std::vector<Seen> g_seen;
std::vector<std::string> g_log;   // what the stubs saw, in order
int g_waits = 0, g_records = 0, g_syncs = 0, g_displays = 0, g_failures = 0;
struct Watch : StubObserver {
    void allocated(void*, size_t) override {}
    void freed(void*) override {}
    void copied(const char* what, void*, const void*, size_t, hipStream_t, bool) override { g_log.push_back(what); }
    void stream_synchronized(hipStream_t) override {}
    void device_synchronized() override {}
    void event_recorded(hipEvent_t, hipStream_t) override { g_records++; g_log.push_back("record"); }
    void event_waited(hipStream_t, hipEvent_t) override { g_waits++; g_log.push_back("wait"); }
    void event_synchronized(hipEvent_t) override { g_syncs++; g_log.push_back("event_sync"); }
    void event_destroyed(hipEvent_t) override {}
};
void expect(bool ok, const char* what) {
    std::printf("%s: %s\n", what, ok ? "ok" : "FAILED");
    if (!ok) g_failures++;
}
bool refused(int rc, const char* word) { return rc == RPT_ERR_INVALID && std::string(rpt_last_error()).find(word) != std::string::npos; }
}  // namespace

namespace rptg {
// Touches what particles_integrate_kernel touches: every state value + 1 per step, the counters + the launch's evaluations.
hipError_t launch_particles_integrate(const ParticlesArgs& a, uint32_t block, uint32_t lanes, hipStream_t st) {
    g_seen.push_back({a, block, lanes, st});
    g_log.push_back("launch");
    for (uint32_t i = 0; i < 3 * a.n; i++) {
        a.pos[i] += double(a.n_steps);
        a.vel[i] -= double(a.n_steps);
    }
    for (int k = 0; k < 6; k++) a.counters[k] += k == 0 ? 4ull * a.n_steps : 1ull;
    return hipSuccess;
}
hipError_t launch_particles_display(const ParticlesArgs& a, double* d_out, hipStream_t) {
    g_displays++;
    g_log.push_back("display");
    for (uint32_t i = 0; i < 3 * a.n; i++) d_out[i] = a.pos[i] * 2.0;
    return hipSuccess;
}
}  // namespace rptg

int main() {
    Watch watch;
    g_stub_observer = &watch;
    hipStream_t const s1 = reinterpret_cast<hipStream_t>(uintptr_t(0x100)), s2 = reinterpret_cast<hipStream_t>(uintptr_t(0x200));
    const uint32_t n = 7;
    const rpt_particles_params prm{RPT_PARTICLES_MARBLES, n, 0.15, 2.0};
    std::vector<double> pos(3 * n, 1.0), vel(3 * n, 2.0), got_p(3 * n), got_v(3 * n);   // exact sizes on the heap

    // ---- life cycle and bad parameters
    rpt_particles_params bad = prm;
    bad.n = 0;
    expect(rpt_particles_create(0, &bad) == nullptr && refused(RPT_ERR_INVALID, "1..256"), "create refuses n = 0");
    bad.n = 257;
    expect(rpt_particles_create(0, &bad) == nullptr, "create refuses n = 257");
    bad = prm;
    bad.radius = 0.0;
    expect(rpt_particles_create(0, &bad) == nullptr && refused(RPT_ERR_INVALID, "radius"), "a marbles system needs a radius");
    bad.kind = 3;
    expect(rpt_particles_create(0, &bad) == nullptr && rpt_particles_create(0, nullptr) == nullptr, "create refuses an unknown kind and NULL");
    expect(rpt_particles_create(3, &prm) == nullptr && refused(RPT_ERR_INVALID, "device"), "create refuses a device that is not there");
    g_stub_malloc_limit = 100;
    expect(rpt_particles_create(0, &prm) == nullptr, "create survives a failed allocation");
    g_stub_malloc_limit = SIZE_MAX;
    rpt_particles_destroy(nullptr);
    rpt_particles* h = rpt_particles_create(0, &prm);
    expect(h && rpt_particles_state(h, got_p.data(), got_v.data()) == RPT_OK && got_p[0] == 0.0 && got_v[3 * n - 1] == 0.0, "a new system's state is zeros");
    expect(rpt_particles_set_state(h, pos.data(), nullptr) == RPT_OK && rpt_particles_state(h, got_p.data(), got_v.data()) == RPT_OK && got_p == pos &&
                   got_v[0] == 0.0 && rpt_particles_set_state(h, pos.data(), vel.data()) == RPT_OK && rpt_particles_state(h, nullptr, got_v.data()) == RPT_OK &&
                   got_v == vel,
           "set_state copies both arrays; NULL velocities are zeros");

    // ---- check order: time, step and the length of the sequence before the handle; a refused call reaches no device call
    g_log.clear();
    expect(refused(rpt_particles_integrate(nullptr, -1.0, 1.0, s1), "time") && refused(rpt_particles_integrate(nullptr, 1.0, 0.0, s1), "step") &&
                   refused(rpt_particles_integrate(h, 1.0 / 0.0, 1.0, s1), "time") && refused(rpt_particles_integrate(h, 1.0, 0.0 / 0.0, s1), "step") &&
                   refused(rpt_particles_integrate(nullptr, 1.0, 1.0, s1), "null"),
           "time and step are checked before the handle");
    expect(refused(rpt_particles_integrate(h, 1048577.0, 1.0, s1), "2^20") && refused(rpt_particles_integrate(h, 1.0, 1e-300, s1), "2^20"),
           "more than 2^20 steps are refused");
    expect(refused(rpt_particles_set_state(nullptr, nullptr, nullptr), "positions") && refused(rpt_particles_set_state(nullptr, pos.data(), nullptr), "system") &&
                   refused(rpt_particles_display_positions(nullptr, nullptr), "output") && refused(rpt_particles_counters(h, nullptr), "output"),
           "the arguments are checked before the handle");
    expect(g_log.empty() && g_seen.empty(), "a refused call reaches no device call");

    // ---- 2,500 steps: 2,499 of 1.0 and one of 0.5, in nine launches of 256 steps and one of 196
    expect(rpt_particles_integrate(h, 2499.5, 1.0, s1) == RPT_OK && g_seen.size() == 10, "2,500 steps are ten launches");
    if (g_seen.size() == 10) {
        const auto &a0 = g_seen[0].a, &a1 = g_seen[8].a, &a2 = g_seen[9].a;
        uint32_t steps = 0, tails = 0;
        for (const Seen& s : g_seen) {
            steps += s.a.n_steps;
            tails += s.a.tail;
        }
        expect(steps == 2500 && tails == 1 && a0.n_steps == 256 && a1.n_steps == 256 && a2.n_steps == 196 && !a0.tail && !a1.tail && a2.tail == 1,
               "at most 256 steps each; the last one has the tail");
        expect(a0.h == 1.0 && a2.h == 1.0 && a2.h_tail == 0.5, "the step and the remainder");
        expect(a0.pos == a2.pos && a0.vel == a2.vel && a0.counters == a2.counters && a0.n == n && a0.kind == RPT_PARTICLES_MARBLES && a0.radius == 0.15 &&
                       a0.height == 2.0 && g_seen[0].st == s1 && g_seen[2].st == s1,
               "every launch works on the handle's arrays, on the caller's stream");
        expect(g_waits == 0 && g_records == 1, "the first call waits for nothing and records the event once");
    }
    expect(rpt_particles_integrate(h, 1048576.0, 1.0, s1) == RPT_OK && g_seen.size() == 10 + 4096 && g_seen.back().a.n_steps == 256 && g_seen.back().a.tail == 1 &&
                   g_seen.back().a.h_tail == 1.0,
           "2^20 steps are accepted: 4096 launches");
    expect(rpt_particles_integrate(h, 0.0, 1.0, s2) == RPT_OK && g_seen.back().a.n_steps == 1 && g_seen.back().a.tail == 1 && g_seen.back().a.h_tail == 0.0 &&
                   g_seen.back().st == s2 && g_waits == 2 && g_records == 3,
           "time 0 is one step of size 0; every call but the first waits for its predecessor's event, whatever its stream");

    // ---- set_state while an integrate is queued: the copy comes after the wait for the handle's event
    g_log.clear();
    const int syncs = g_syncs;
    expect(rpt_particles_integrate(h, 1.5, 1.0, s1) == RPT_OK && rpt_particles_set_state(h, pos.data(), vel.data()) == RPT_OK && g_syncs == syncs + 1 &&
                   g_log.size() == 6 && g_log[0] == "wait" && g_log[1] == "launch" && g_log[2] == "record" && g_log[3] == "event_sync" && g_log[4] == "hipMemcpy",
           "set_state waits for the queued integrate before it copies");
    expect(rpt_particles_state(h, got_p.data(), got_v.data()) == RPT_OK && got_p == pos && got_v == vel, "... and its state is the one that stays");
    expect(rpt_particles_integrate(h, 2.5, 1.0, nullptr) == RPT_OK && rpt_particles_state(h, got_p.data(), got_v.data()) == RPT_OK && got_p[0] == 4.0 &&
                   got_v[3 * n - 1] == -1.0,
           "the next integrate starts from it");

    // ---- counters, display positions, the device arrays
    uint64_t c[8];
    const uint64_t launches = g_seen.size();
    expect(rpt_particles_counters(h, c) == RPT_OK && c[0] == 4ull * (2500 + 1048576 + 1 + 2 + 3) && c[1] == launches && c[6] == launches && c[7] == 0,
           "the counters add up over the launches; 6 is the number of launches");
    expect(rpt_particles_display_positions(h, got_p.data()) == RPT_OK && got_p[0] == 8.0 && g_displays == 1 && rpt_particles_counters(h, c) == RPT_OK &&
                   c[6] == launches + 1,
           "display positions: one launch, n * 3 doubles back");
    void *dp = nullptr, *dv = nullptr;
    expect(rpt_particles_state_device(h, &dp, &dv) == RPT_OK && dp == g_seen.back().a.pos && dv == g_seen.back().a.vel, "state_device hands out the handle's arrays");
    const rpt_particles_params grav{RPT_PARTICLES_GRAVITY, 2, 0.0, 0.0};
    rpt_particles* g = rpt_particles_create(0, &grav);
    expect(g && rpt_particles_display_positions(g, got_p.data()) == RPT_ERR_UNSUPPORTED && g_displays == 1, "display positions of another system: RPT_ERR_UNSUPPORTED");
    rpt_particles_destroy(g);
    rpt_particles_destroy(h);
    g_stub_observer = nullptr;
    std::printf("launches=%zu waits=%d records=%d failures=%d\n", g_seen.size(), g_waits, g_records, g_failures);
    return g_failures ? 1 : 0;
}

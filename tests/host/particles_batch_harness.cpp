// Test infrastructure for tests/test_host_particles_batch.py: the host half of rpt_particles_batch_* in the real
// rpt_amd/csrc/rpt_particles.cpp over malloc-backed HIP stubs (hip_stubs.h), run as a program of its own under AddressSanitizer +
// UBSan and plain.  The stubs of the two batch launchers read the device table and read and write every byte the kernels would (each
// system's slice of both state arrays, its six counters, its slice of the display array), so an array that is too small, a wrong
// first-particle index or a freed table is a sanitizer report; they record their arguments.  The resident-block function is replaced
// (g_resident), so main() checks the launch rule for an R of its choice.  main() checks the life cycle, a failed allocation at each
// allocation, every refusal in its stated order, the cut of a 2,500-step sequence at R = 4 for 1, 4, 5, 9 and 1,025 systems, the
// event that orders the calls of one batch, and a set_system_state issued while an integrate is queued; it prints the table the
// host built for mixed sizes ("table ..." lines, which the Python test compares with numpy).  One line per check; exit code 1 on a
// failure.
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
    rptg::ParticlesBatchArgs a;
    uint32_t block, lanes;
    hipStream_t st;
};
std::vector<Seen> g_seen;
std::vector<std::string> g_log;   // what the stubs saw, in order
int g_waits = 0, g_records = 0, g_syncs = 0, g_displays = 0, g_failures = 0;
uint32_t g_resident = 4;
int g_allocations = 0, g_fail_after = -1;   // >= 0: the allocation after that many fails
struct Watch : StubObserver {
    void allocated(void*, size_t) override {
        g_allocations++;
        if (g_fail_after >= 0 && g_allocations >= g_fail_after) g_stub_malloc_limit = 0;
    }
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
bool said(const char* word) { return std::string(rpt_last_error()).find(word) != std::string::npos; }
bool refused(int rc, const char* word) { return rc == RPT_ERR_INVALID && said(word); }
std::vector<rpt_particles_params> marbles_of(const std::vector<uint32_t>& sizes) {
    std::vector<rpt_particles_params> p;
    for (uint32_t n : sizes) p.push_back({RPT_PARTICLES_MARBLES, n, 0.15, 2.0});
    return p;
}
}  // namespace

namespace rptg {
// Touches what particles_batch_integrate_kernel touches, block by block through the table: every state value of system s + 1 per
// step, its counters + the launch's evaluations.
hipError_t launch_particles_batch_integrate(const ParticlesBatchArgs& a, uint32_t block, uint32_t lanes, hipStream_t st) {
    g_seen.push_back({a, block, lanes, st});
    if (g_log.size() < 64) g_log.push_back("launch");
    for (uint32_t s = 0; s < a.n_systems; s++) {
        const ParticlesSystemRecord r = a.table[s];
        for (uint32_t i = 0; i < 3 * r.n; i++) {
            a.pos[3 * size_t(r.first) + i] += double(a.n_steps);
            a.vel[3 * size_t(r.first) + i] -= double(a.n_steps);
        }
        for (int k = 0; k < 6; k++) a.counters[8 * size_t(s) + k] += k == 0 ? 4ull * a.n_steps : 1ull;
    }
    return hipSuccess;
}
hipError_t launch_particles_batch_display(const ParticlesBatchArgs& a, double* d_out, hipStream_t) {
    g_displays++;
    g_log.push_back("display");
    for (uint32_t s = 0; s < a.n_systems; s++) {
        const ParticlesSystemRecord r = a.table[s];
        for (uint32_t i = 0; i < 3 * r.n; i++) d_out[3 * size_t(r.first) + i] = a.pos[3 * size_t(r.first) + i] * 2.0;
    }
    return hipSuccess;
}
hipError_t particles_batch_resident_blocks(int, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t* resident) {
    *resident = g_resident;
    return hipSuccess;
}
hipError_t launch_particles_integrate(const ParticlesArgs&, uint32_t, uint32_t, hipStream_t) { return hipErrorInvalidValue; }
hipError_t launch_particles_display(const ParticlesArgs&, double*, hipStream_t) { return hipErrorInvalidValue; }
}  // namespace rptg

namespace {
// The table the host built for `sizes`: the first-particle indices as the device array and as the records say, the dynamic LDS bytes.
void print_table(const std::vector<uint32_t>& sizes) {
    const auto prm = marbles_of(sizes);
    rpt_particles_batch* b = rpt_particles_batch_create(0, prm.data(), uint32_t(prm.size()));
    void* d_first = nullptr;
    uint64_t info[8] = {};
    bool ok = b && rpt_particles_batch_state_device(b, nullptr, nullptr, &d_first) == RPT_OK && rpt_particles_batch_info(b, info) == RPT_OK;
    std::string s_n, s_first;
    for (size_t s = 0; ok && s < sizes.size(); s++) {
        const uint32_t f = static_cast<const uint32_t*>(d_first)[s];
        const rptg::ParticlesSystemRecord& r = b->d_table.get<rptg::ParticlesSystemRecord>()[s];
        ok = ok && r.first == f && r.n == sizes[s] && r.kind == RPT_PARTICLES_MARBLES && r.radius == 0.15 && r.height == 2.0;
        s_n += (s ? "," : "") + std::to_string(sizes[s]);
        s_first += (s ? "," : "") + std::to_string(f);
    }
    std::printf("table sizes=%s first=%s lds=%llu n_max=%llu total=%llu %s\n", s_n.c_str(), s_first.c_str(), (unsigned long long)info[3], (unsigned long long)info[4],
                (unsigned long long)info[5], ok ? "ok" : "FAILED");
    if (!ok) g_failures++;
    rpt_particles_batch_destroy(b);
}
// 2,500 steps (2,499 of 1.0 and one of 0.5) on a batch of `n_systems` systems of 2 or 3 particles at R = g_resident
void launch_rule(uint32_t n_systems) {
    std::vector<uint32_t> sizes(n_systems);
    for (uint32_t s = 0; s < n_systems; s++) sizes[s] = 2 + s % 2;
    const auto prm = marbles_of(sizes);
    rpt_particles_batch* b = rpt_particles_batch_create(0, prm.data(), n_systems);
    const uint32_t rounds = (n_systems + g_resident - 1) / g_resident, scaled = rounds * rptg::kBatchLaunchScale;
    const uint32_t L = 256 / scaled < 1 ? 1 : 256 / scaled, want = (2500 + L - 1) / L;
    g_seen.clear();
    uint64_t info[8] = {};
    bool ok = b && rpt_particles_batch_info(b, info) == RPT_OK && info[0] == g_resident && info[1] == rounds && info[2] == L &&
              rpt_particles_batch_integrate(b, 2499.5, 1.0, nullptr) == RPT_OK && g_seen.size() == want;
    uint32_t steps = 0;
    for (size_t i = 0; ok && i < g_seen.size(); i++) {
        const auto& a = g_seen[i].a;
        const bool last = i + 1 == g_seen.size();
        ok = a.n_systems == n_systems && a.n_max == (n_systems > 1 ? 3u : 2u) && a.h == 1.0 && a.h_tail == 0.5 && a.tail == (last ? 1u : 0u) &&
             (last ? a.n_steps >= 1 && a.n_steps <= L : a.n_steps == L);
        steps += a.n_steps;
    }
    ok = ok && steps == 2500;
    std::vector<uint64_t> c(8 * size_t(n_systems));
    std::vector<double> p(3 * size_t(info[5]));
    ok = ok && rpt_particles_batch_counters(b, c.data()) == RPT_OK && rpt_particles_batch_state(b, p.data(), nullptr) == RPT_OK && p.front() == 2500.0 &&
         p.back() == 2500.0;
    for (uint32_t s = 0; ok && s < n_systems; s++) ok = c[8 * s] == 10000 && c[8 * s + 1] == want && c[8 * s + 6] == want && c[8 * s + 7] == 0;
    std::printf("launch rule: %u systems at R = %u: %u rounds, %u steps a launch, %zu launches, the tail on the last only: %s\n", n_systems, g_resident, rounds, L,
                g_seen.size(), ok ? "ok" : "FAILED");
    if (!ok) g_failures++;
    rpt_particles_batch_destroy(b);
}
}  // namespace

int main() {
    Watch watch;
    g_stub_observer = &watch;
    hipStream_t const s1 = reinterpret_cast<hipStream_t>(uintptr_t(0x100)), s2 = reinterpret_cast<hipStream_t>(uintptr_t(0x200));
    const std::vector<uint32_t> sizes{7, 1, 25};
    const uint32_t total = 33;
    std::vector<rpt_particles_params> prm = marbles_of(sizes);
    std::vector<double> pos(3 * total, 1.0), vel(3 * total, 2.0), got_p(3 * total), got_v(3 * total);   // exact sizes on the heap

    // ---- refusals, in their stated order; none reaches a device call
    g_log.clear();
    expect(rpt_particles_batch_create(0, nullptr, 0) == nullptr && said("null particle parameters"), "create: NULL parameters come first");
    std::vector<rpt_particles_params> bad = prm;
    bad[1].n = 0;
    expect(rpt_particles_batch_create(0, bad.data(), 0) == nullptr && said("1..4096") && rpt_particles_batch_create(0, bad.data(), 4097) == nullptr && said("1..4096"),
           "create refuses 0 and 4097 systems, before it looks at a system");
    expect(rpt_particles_batch_create(0, bad.data(), 3) == nullptr && said("system 1:") && said("1..256"), "a bad system in the middle is named by its index");
    bad[2].radius = 0.0;
    expect(rpt_particles_batch_create(0, bad.data(), 3) == nullptr && said("system 1:"), "of two bad systems the first is named");
    bad[1].n = 257;
    expect(rpt_particles_batch_create(3, bad.data(), 3) == nullptr && said("system 1:") && said("1..256"), "the systems are checked before the device");
    bad[1].n = 1;
    expect(rpt_particles_batch_create(0, bad.data(), 3) == nullptr && said("system 2:") && said("radius"), "a marbles system needs a radius");
    bad[2].kind = 3;
    expect(rpt_particles_batch_create(0, bad.data(), 3) == nullptr && said("system 2:") && said("kind"), "an unknown kind");
    expect(rpt_particles_batch_create(3, prm.data(), 3) == nullptr && said("device"), "create refuses a device that is not there");
    expect(g_log.empty() && g_allocations == 0, "a refused create reaches no device call");

    // ---- a failed allocation at each allocation
    int failed = 0;
    for (int k = 0; k < 16; k++) {
        g_allocations = 0;
        g_fail_after = k;
        if (k == 0) g_stub_malloc_limit = 0;
        rpt_particles_batch* b = rpt_particles_batch_create(0, prm.data(), 3);
        g_fail_after = -1;
        g_stub_malloc_limit = SIZE_MAX;
        if (b) {
            rpt_particles_batch_destroy(b);
            break;
        }
        failed++;
    }
    expect(failed == 6, "create survives a failed allocation at each of its six allocations");
    g_log.clear();

    // ---- life cycle
    rpt_particles_batch_destroy(nullptr);
    rpt_particles_batch* h = rpt_particles_batch_create(0, prm.data(), 3);
    expect(h && rpt_particles_batch_state(h, got_p.data(), got_v.data()) == RPT_OK && got_p[0] == 0.0 && got_v[3 * total - 1] == 0.0, "a new batch's state is zeros");
    expect(rpt_particles_batch_set_state(h, pos.data(), nullptr) == RPT_OK && rpt_particles_batch_state(h, got_p.data(), got_v.data()) == RPT_OK && got_p == pos &&
                   got_v[0] == 0.0 && rpt_particles_batch_set_state(h, pos.data(), vel.data()) == RPT_OK &&
                   rpt_particles_batch_state(h, nullptr, got_v.data()) == RPT_OK && got_v == vel,
           "set_state copies both arrays; NULL velocities are zeros");
    {
        std::vector<double> one_p(3, 5.0), one_v(3, 6.0);   // system 1: one particle, at particle index 7
        expect(rpt_particles_batch_set_system_state(h, 1, one_p.data(), one_v.data()) == RPT_OK && rpt_particles_batch_state(h, got_p.data(), got_v.data()) == RPT_OK &&
                       got_p[20] == 1.0 && got_p[21] == 5.0 && got_p[23] == 5.0 && got_p[24] == 1.0 && got_v[21] == 6.0 && got_v[24] == 2.0 &&
                       rpt_particles_batch_set_system_state(h, 1, one_p.data(), nullptr) == RPT_OK && rpt_particles_batch_state(h, nullptr, got_v.data()) == RPT_OK &&
                       got_v[20] == 2.0 && got_v[21] == 0.0 && got_v[23] == 0.0 && got_v[24] == 2.0,
               "set_system_state writes one system's slice and nothing else");
        std::vector<double> last_p(75, 1.0), last_v(75, 2.0);   // system 2: exactly 25 particles, to the end of the arrays
        expect(rpt_particles_batch_set_system_state(h, 2, last_p.data(), last_v.data()) == RPT_OK && rpt_particles_batch_set_state(h, pos.data(), vel.data()) == RPT_OK,
               "... the last system's ends where the arrays end");
    }

    // ---- check order of the other calls; a refused call reaches no device call
    g_log.clear();
    uint64_t info8[8];
    expect(refused(rpt_particles_batch_integrate(nullptr, -1.0, 1.0, s1), "time") && refused(rpt_particles_batch_integrate(nullptr, 1.0, 0.0, s1), "step") &&
                   refused(rpt_particles_batch_integrate(h, 1.0 / 0.0, 1.0, s1), "time") && refused(rpt_particles_batch_integrate(h, 1.0, 0.0 / 0.0, s1), "step") &&
                   refused(rpt_particles_batch_integrate(nullptr, 1.0, 1.0, s1), "null"),
           "time and step are checked before the batch");
    expect(refused(rpt_particles_batch_integrate(h, 1048577.0, 1.0, s1), "2^20") && refused(rpt_particles_batch_integrate(h, 1.0, 1e-300, s1), "2^20"),
           "more than 2^20 steps are refused");
    expect(refused(rpt_particles_batch_set_state(nullptr, nullptr, nullptr), "positions") && refused(rpt_particles_batch_set_state(nullptr, pos.data(), nullptr), "ensemble") &&
                   refused(rpt_particles_batch_set_system_state(nullptr, 9, nullptr, nullptr), "positions") &&
                   refused(rpt_particles_batch_set_system_state(nullptr, 9, pos.data(), nullptr), "ensemble") &&
                   refused(rpt_particles_batch_set_system_state(h, 3, pos.data(), nullptr), "system index") &&
                   refused(rpt_particles_batch_set_system_state(h, 0xffffffffu, pos.data(), nullptr), "system index") &&
                   refused(rpt_particles_batch_display_positions(nullptr, nullptr), "output") && refused(rpt_particles_batch_counters(h, nullptr), "output") &&
                   refused(rpt_particles_batch_state(h, nullptr, nullptr), "outputs") && refused(rpt_particles_batch_state_device(h, nullptr, nullptr, nullptr), "outputs") &&
                   refused(rpt_particles_batch_info(h, nullptr), "output") && refused(rpt_particles_batch_info(nullptr, info8), "ensemble"),
           "the arguments are checked before the batch, a system index against its number of systems");
    {
        std::vector<rpt_particles_params> mixed = prm;
        mixed[1] = {RPT_PARTICLES_GRAVITY, 2, 0.0, 0.0};
        rpt_particles_batch* g = rpt_particles_batch_create(0, mixed.data(), 3);
        g_log.clear();
        std::vector<double> out(3 * 34);
        expect(g && rpt_particles_batch_display_positions(g, out.data()) == RPT_ERR_UNSUPPORTED && said("marbles") && g_displays == 0 && g_log.empty(),
               "display positions of a batch with one system that is not MARBLES: RPT_ERR_UNSUPPORTED");
        rpt_particles_batch_destroy(g);
    }
    expect(g_log.empty() && g_seen.empty(), "a refused call reaches no device call");

    // ---- the launch rule at R = 4
    for (uint32_t n_systems : {1u, 4u, 5u, 9u, 1025u}) launch_rule(n_systems);
    g_seen.clear();
    g_log.clear();

    // ---- the event that orders the calls of one batch, whatever their streams
    g_waits = g_records = 0;
    expect(rpt_particles_batch_integrate(h, 2.5, 1.0, s1) == RPT_OK && g_waits == 0 && g_records == 1 && g_seen.size() == 1 && g_seen[0].a.n_steps == 3 &&
                   g_seen[0].a.tail == 1 && g_seen[0].a.h_tail == 0.5 && g_seen[0].st == s1 && g_seen[0].a.n_max == 25 && g_seen[0].a.n_systems == 3,
           "the first call waits for nothing and records the event once");
    expect(rpt_particles_batch_integrate(h, 0.0, 1.0, s2) == RPT_OK && g_seen.back().a.n_steps == 1 && g_seen.back().a.tail == 1 && g_seen.back().a.h_tail == 0.0 &&
                   g_seen.back().st == s2 && g_waits == 1 && g_records == 2 && rpt_particles_batch_integrate(h, 1.0, 1.0, s1) == RPT_OK && g_waits == 2 && g_records == 3,
           "time 0 is one step of size 0; every call but the first waits for its predecessor's event, whatever its stream");

    // ---- set_system_state while an integrate is queued: the copy comes after the wait for the batch's event
    g_log.clear();
    const int syncs = g_syncs;
    std::vector<double> sp(21, 9.0), sv(21, -9.0);
    expect(rpt_particles_batch_integrate(h, 1.5, 1.0, s1) == RPT_OK && rpt_particles_batch_set_system_state(h, 0, sp.data(), sv.data()) == RPT_OK && g_syncs == syncs + 1 &&
                   g_log.size() == 6 && g_log[0] == "wait" && g_log[1] == "launch" && g_log[2] == "record" && g_log[3] == "event_sync" && g_log[4] == "hipMemcpy" &&
                   g_log[5] == "hipMemcpy",
           "set_system_state waits for the queued integrate before it copies");
    expect(rpt_particles_batch_state(h, got_p.data(), got_v.data()) == RPT_OK && got_p[0] == 9.0 && got_p[20] == 9.0 && got_v[20] == -9.0 && got_p[21] == 1.0 + 3 + 1 + 1 + 2,
           "... its state is the one that stays, and the other systems keep theirs");
    expect(rpt_particles_batch_integrate(h, 2.5, 1.0, nullptr) == RPT_OK && rpt_particles_batch_state(h, got_p.data(), got_v.data()) == RPT_OK && got_p[0] == 12.0 &&
                   got_v[20] == -12.0,
           "the next integrate starts from it");

    // ---- counters, display positions, the device arrays
    std::vector<uint64_t> c(24);
    const uint64_t launches = g_seen.size();
    expect(rpt_particles_batch_counters(h, c.data()) == RPT_OK && c[0] == 4ull * (3 + 1 + 1 + 2 + 3) && c[16] == c[0] && c[1] == launches && c[6] == launches &&
                   c[8 + 6] == launches && c[16 + 6] == launches && c[7] == 0 && c[23] == 0,
           "each system's counters add up over the launches; 6 is the number of launches");
    expect(rpt_particles_batch_display_positions(h, got_p.data()) == RPT_OK && got_p[0] == 24.0 && got_p[3 * total - 1] == 2.0 * (1.0 + 10) && g_displays == 1 &&
                   rpt_particles_batch_counters(h, c.data()) == RPT_OK && c[6] == launches + 1,
           "display positions: one launch, sum(n) * 3 doubles back");
    void *dp = nullptr, *dv = nullptr, *df = nullptr;
    expect(rpt_particles_batch_state_device(h, &dp, &dv, &df) == RPT_OK && dp == g_seen.back().a.pos && dv == g_seen.back().a.vel && df &&
                   static_cast<uint32_t*>(df)[0] == 0 && static_cast<uint32_t*>(df)[1] == 7 && static_cast<uint32_t*>(df)[2] == 8,
           "state_device hands out the batch's arrays and the first-particle indices");
    rpt_particles_batch_destroy(h);

    // ---- the table for mixed sizes, 56 | 57 included
    for (const std::vector<uint32_t>& s : {std::vector<uint32_t>{1, 56, 3}, std::vector<uint32_t>{57, 2, 25, 1}, std::vector<uint32_t>{256, 1, 256},
                                           std::vector<uint32_t>{5}, std::vector<uint32_t>{2, 3, 2, 3, 2}})
        print_table(s);
    g_stub_observer = nullptr;
    std::printf("waits=%d records=%d displays=%d failures=%d\n", g_waits, g_records, g_displays, g_failures);
    return g_failures ? 1 : 0;
}
